"""bench.py --dump-outputs and the plain / --full split: the last timed step's result is written as float64
arrays that depend on the arguments alone, and a plain run carries none of the legs that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class PlantedCtx:
    """Stand-in for _lib.Context: one planted hit index, the stats fields run_workload reads."""

    def __init__(self, hit):
        self.hit = hit

    def search_range(self, cs, pwlen, start, n, stop_on_first=False, cap=1 << 16):
        hits = [self.hit] if start <= self.hit < start + n else []
        return hits, len(hits), {"candidates": n, "wall_ms": 1.0}


def _dump(tmp_path, tag, hit, steps=3, warmup=2):
    import bench
    last = {}
    bench.run_workload("office", PlantedCtx(hit), 0, 1, steps, warmup, lambda: None, lambda v: v, batch=1000, last=last)
    out = tmp_path / tag
    bench.dump_outputs(str(out), last)
    return {f[:-4]: np.load(str(out / f)) for f in sorted(os.listdir(str(out)))}


def test_dump_outputs_is_the_last_timed_step(tmp_path):
    # steps 2..4 are timed (2 warmup steps), windows of 1000 from index step * 1000: the last one is [4000, 5000)
    a = _dump(tmp_path, "a", hit=4321)
    assert sorted(a) == ["candidates", "lowest_hit_index", "window"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["window"].tolist() == [4000.0, 1000.0]
    assert a["candidates"].tolist() == [1000.0]
    assert a["lowest_hit_index"].tolist() == [4321.0]
    # a hit of an earlier timed step is not the last step's output; no hit is -1
    assert _dump(tmp_path, "b", hit=3500)["lowest_hit_index"].tolist() == [-1.0]
    # --steps sets the number of timed steps: one fewer ends one window earlier
    assert _dump(tmp_path, "c", hit=3500, steps=2)["lowest_hit_index"].tolist() == [3500.0]
    # same arguments, same files
    a2 = _dump(tmp_path, "a2", hit=4321)
    assert all(np.array_equal(a[k], a2[k]) for k in a)


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    """One plain run of the Office workload (one 26^4 batch per step): the result line's contract fields, none of
    the --full legs, and the dump of the last step."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--workload", "office", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["unit"] == "candidates/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] == pytest.approx(26 ** 4 / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert d["per_format"] == {} and d["cpu_baseline"] is None and d["cluster"] is None
    assert d["roofline"]["kernel"] == "k_office_kdf"
    got = {f: np.load(str(out / f)) for f in sorted(os.listdir(str(out)))}
    assert sorted(got) == ["candidates.npy", "lowest_hit_index.npy", "window.npy"]
    assert got["candidates.npy"].tolist() == [float(26 ** 4)]
    assert got["lowest_hit_index.npy"].tolist() == [-1.0]      # the document's password has 8 characters
