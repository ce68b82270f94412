"""bench.py's plain run and --dump-outputs (the benchmark's own command line, so the
test starts it): a plain run times its steps and prints the line without any check
against the oracle or extra leg; --dump-outputs writes what the last timed step
computed, the same files from run to run, and the right values."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tcbee_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = 300_000  # more records than bench.DUMP_SAMPLE (65536): the outputs are sampled
FLOWS = 2_000
ORACLE_KEYS = ("full_bit_exact", "sample_bit_exact", "flow_table_exact", "flows", "pkts_total")
FULL_LEGS = ("cpu_baseline", "e2e_host", "config5_replay", "config2_1M_64B", "config3_zipf",
             "config3_ipv6", "config3_warm_table", "config4_shard_1M_flows",
             "config4_flowhash_share_of_8")


def run_bench(args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--frames", str(FRAMES),
                        "--flows", str(FLOWS)] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def test_plain_run_and_dump_outputs(gpu, oracle, tmp_path):
    dirs = [str(tmp_path / d) for d in ("a", "b")]
    outs = [run_bench(["--steps", "3", "--warmup", "1", "--dump-outputs", d]) for d in dirs]
    for out, err in outs:
        # the plain line: the headline figures, nothing checked against the oracle,
        # no other leg
        assert out["steps"] == 3 and out["warmup"] == 1
        assert out["ms_per_step"] > 0 and out["unit"] == "Mpkt/s" and out["dtype"] == "u8"
        assert out["higher_is_better"] is True
        # value = frames x steps / elapsed, ms_per_step = elapsed / steps
        # (the line rounds ms_per_step to 1e-4 ms: up to 0.5 % of a >= 0.01 ms step)
        assert out["value"] == pytest.approx(FRAMES / out["ms_per_step"] / 1e3, rel=1e-2)
        assert out["check"]["records"] == FRAMES and out["check"]["status"] == 0
        assert not [k for k in ORACLE_KEYS if k in out["check"]]
        assert not [k for k in FULL_LEGS if k in out]
        assert "validating" not in err and "cpu baseline" not in err
    # the files: float32 / float64, at most 64 MB in all, identical from run to run
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert set(names) == {n + ".npy" for n in ("record_index", "records", "flow_hash", "flow_id",
                                                "n_records", "counters", "flow_index",
                                                "flow_table")}
    a = {n[:-4]: np.load(os.path.join(dirs[0], n)) for n in names}
    b = {n[:-4]: np.load(os.path.join(dirs[1], n)) for n in names}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # and they hold what the step computed: the sampled rows equal the oracle's
    tr = tcbee_amd.synth_trace(FRAMES, sizes="imix", kind=1, n_flows=FLOWS, seed=0x7CBEE)
    rec, fh, fi, ctr, table = oracle.parse(tr)
    idx = a["record_index"].astype(np.int64)
    # 65536 draws with replacement from 300k rows: n (1 - exp(-k / n)) = 58.9k distinct
    # rows expected (standard deviation ~ 0.2k), plus the first and last row
    assert 57_000 < len(idx) <= 65_538 and idx[0] == 0 and idx[-1] == FRAMES - 1
    assert np.all(np.diff(idx) > 0)
    assert a["n_records"][0] == FRAMES == len(rec)
    assert np.array_equal(a["records"], rec[idx].astype(np.float32))
    assert np.array_equal(a["flow_hash"], fh[idx].astype(np.float64))
    assert np.array_equal(a["flow_id"], fi[idx].astype(np.float64))
    # (the counters are added to across the 1 warm-up + 3 timed steps of one buffer)
    assert a["counters"].tolist() == [4 * ctr[k] for k in ("ingress", "egress", "handled",
                                                           "dropped")]
    assert np.array_equal(a["flow_index"], np.arange(len(table)))
    assert np.array_equal(a["flow_table"],
                          table.view(np.uint8).reshape(len(table), 64).astype(np.float32))


def test_full_run_checks_against_the_oracle(gpu):
    out, err = run_bench(["--steps", "2", "--warmup", "1", "--full", "--no-extra", "--no-cpu"])
    assert out["check"]["full_bit_exact"] is True and out["check"]["flow_table_exact"] is True
    assert out["check"]["flows"] == FLOWS and out["check"]["full_records"] == FRAMES
    assert "validating" in err
