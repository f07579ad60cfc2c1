"""bench.py's plain / --full split and --dump-outputs.

CPU: run_rank over the oracle-backed engine double of test_bench_ranks (a plain run makes no call
beyond warmup + steps; --full adds the 3 probe steps and stages_ms), and dump_outputs over a host
batch (whole arrays when small, the same ascending seeded sample when large).  GPU: one small
`bench.py --dump-outputs` process, its files against the oracle's redaction of the same corpus."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
from test_bench_ranks import ARGS, OracleBenchEngine, _shard_rows

SPAN_FIELDS = ["utt", "start", "end", "info_type", "likelihood", "flags"]


class CountingEngine(OracleBenchEngine):
    calls = 0
    levels = ()

    def scan_redact_device(self, *a):
        super().scan_redact_device(*a)
        self.calls += 1

    scan_redact_device_ex = scan_redact_device

    def set_timing(self, level):
        self.levels += (level,)


@pytest.mark.parametrize("full", [False, True])
def test_run_rank_plain_and_full(full, oracle_cfg):
    import bench
    args = argparse.Namespace(**ARGS, full=full)
    made = []

    def make_engine(batch, bank, C):
        made.append(CountingEngine(_shard_rows(0, C, args.utt_per_conv, args.bank), oracle_cfg))
        return made[-1]
    line = bench.run_rank(args, 0, 1, torch.device("cpu"), make_engine)
    eng, = made
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == ARGS["steps"] and line["ms_per_step"] > 0 and line["histogram"]["verified"] is True
    if full:
        assert eng.calls == ARGS["warmup"] + ARGS["steps"] + 3 and eng.levels == (2, 1)
        assert set(line["stages_ms"]) == {"scan+pairs", "context", "resolve", "offsets", "redact", "pipeline"}
    else:
        assert eng.calls == ARGS["warmup"] + ARGS["steps"] and eng.levels == ()
        assert "stages_ms" not in line and line["cpu_baseline"] is None


class HostBatch:
    def __init__(self, n, out_bytes, n_spans, seed=0):
        r = np.random.default_rng(seed)
        self.n = n
        self.out = torch.from_numpy(r.integers(0, 256, out_bytes + 7, dtype=np.uint8))
        self.out_offs = torch.from_numpy(np.sort(r.integers(0, out_bytes, n + 1)).astype(np.int64))
        self.ctx = torch.from_numpy(r.integers(-1, 40, n).astype(np.int16))
        self.spans = torch.from_numpy(r.integers(0, 256, (n_spans + 3) * 16, dtype=np.uint8))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_arrays(tmp_path):
    import bench
    E = pkg("engine")
    B = HostBatch(50, 4000, 31)
    hist = np.arange(9)
    bench.dump_outputs(str(tmp_path / "d"), B, 4000, 31, hist)
    a = _load(str(tmp_path / "d"))
    assert sorted(a) == ["ctx", "histogram", "out_bytes", "out_offs", "spans", "totals"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert (a["out_bytes"] == B.out.numpy()[:4000]).all() and (a["out_offs"] == B.out_offs.numpy()).all()
    assert (a["ctx"] == B.ctx.numpy()).all() and (a["histogram"] == hist).all() and a["totals"].tolist() == [4000, 31]
    want = B.spans.numpy()[:31 * 16].view(E.SPAN_DTYPE)
    assert a["spans"].shape == (31, 6)
    for j, f in enumerate(SPAN_FIELDS):
        assert (a["spans"][:, j] == want[f]).all()


def test_dump_outputs_sampled_is_repeatable(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_ROWS", 16)
    monkeypatch.setattr(bench, "DUMP_BYTES", 100)
    monkeypatch.setattr(bench, "DUMP_SPANS", 8)
    B = HostBatch(50, 4000, 31)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), B, 4000, 31, np.arange(9))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert all((a[k] == b[k]).all() for k in a)
    assert a["out_offs"].shape == a["ctx"].shape == (16,) and a["out_bytes"].shape == (100,)
    assert a["spans"].shape == (8, 6)
    # the sample is ascending positions of the whole array
    assert (np.diff(a["out_offs"]) >= 0).all()
    assert np.isin(a["out_offs"], B.out_offs.numpy()).all()
    # another output at the sampled positions shows up in the dump
    B2 = HostBatch(50, 4000, 31, seed=1)
    bench.dump_outputs(str(tmp_path / "c"), B2, 4000, 31, np.arange(9))
    assert not (_load(str(tmp_path / "c"))["out_bytes"] == a["out_bytes"]).all()


@pytest.mark.gpu
def test_bench_dump_outputs_matches_oracle(tmp_path, oracle_cfg):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR` on a 12 x 10 utterance corpus: the
    result line's fields, and every dumped array against oracle.process_rows of the same rows."""
    from oracle import pii_oracle as O
    C, U, bank_n = 12, 10, 200
    d = str(tmp_path / "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--conversations", str(C), "--utt-per-conv", str(U), "--bank", str(bank_n),
                        "--dump-outputs", d], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "MB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8" and "stages_ms" not in line
    assert line["cpu_baseline"] is None
    a = _load(d)
    rows = _shard_rows(0, C, U, bank_n)
    exp = O.process_rows(rows, oracle_cfg)
    red = b"".join(r[0] for r in exp)
    offs = np.concatenate([[0], np.cumsum([len(r[0]) for r in exp])])
    spans = [(i, f.start, f.end, f.type_id, f.likelihood) for i, r in enumerate(exp) for f in r[1]]
    assert a["totals"].tolist() == [len(red), len(spans)] and len(spans) > 0
    assert a["out_bytes"].astype(np.uint8).tobytes() == red
    assert (a["out_offs"] == offs).all()
    assert a["spans"][:, :5].astype(np.int64).tolist() == [list(s) for s in spans]
    T = len(oracle_cfg.type_names)
    assert a["histogram"][T] == len(spans)
    assert (a["histogram"][:T] == np.bincount([s[3] for s in spans], minlength=T)).all()
    assert a["ctx"].shape == (C * U,)
