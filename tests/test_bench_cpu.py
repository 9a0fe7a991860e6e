"""CPU: the argument plumbing of bench.py -- `--gpus N` starts its own ranks.

The contract verb is `python bench.py --gpus N`; under a launcher (WORLD_SIZE set) the process is a rank, without one and
with N > 1 it starts `torch.distributed.run --nproc-per-node N bench.py <same arguments>` as a CHILD (never an exec, and
before torch or HIP has been touched) and hands its exit code on.  No GPU here: the ranks themselves end with
"needs an MI355X", which is what the end-to-end case below looks for."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_a_single_rank_goes_on():
    assert bench.launch_ranks(1, [], environ={}) is None
    assert bench.launch_ranks(1, ["--steps", "3"], environ={"WORLD_SIZE": "1"}) is None


def test_under_a_launcher_the_process_is_a_rank():
    called = []
    assert bench.launch_ranks(8, ["--gpus", "8"], environ={"WORLD_SIZE": "8", "RANK": "3"}, run=lambda *a, **k: called.append(a)) is None
    assert not called


def test_world_size_and_gpus_must_agree(capsys):
    assert bench.launch_ranks(8, ["--gpus", "8"], environ={"WORLD_SIZE": "1"}) == 2
    assert bench.launch_ranks(1, [], environ={"WORLD_SIZE": "2"}) == 2
    assert "WORLD_SIZE" in capsys.readouterr().err


def test_gpus_n_without_a_launcher_starts_n_ranks():
    seen = {}

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    rc = bench.launch_ranks(4, argv, environ={"PATH": os.environ.get("PATH", ""), "TDOA_BENCH_BACKEND": "gloo"}, run=fake_run)
    assert rc == 7                                                # the child's exit code is the parent's
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == argv                                    # the same arguments, --gpus included
    assert seen["env"]["TDOA_BENCH_BACKEND"] == "gloo" and "WORLD_SIZE" not in seen["env"]


def test_a_given_master_port_is_kept():
    seen = {}
    bench.launch_ranks(2, [], environ={"MASTER_PORT": "29777"}, run=lambda cmd, env=None: seen.setdefault("cmd", cmd) and 0)
    assert seen["cmd"][seen["cmd"].index("--master-port") + 1] == "29777"


def test_end_to_end_without_a_gpu_the_ranks_start_and_refuse():
    """`python bench.py --gpus 2` here: two ranks come up under torch.distributed.run, each finds no HIP device and says so;
    the parent hands the launcher's non-zero status on and prints no JSON line.  The children see no device on a GPU machine
    either (a negative ordinal ends the visible list), so there too nothing they start runs on the GPU."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0
    assert "starting 2 ranks" in r.stderr and "needs an MI355X" in r.stderr
    assert r.stdout.strip() == ""


def _peaks(n_windows, n_pairs):
    import numpy as np
    import tdoa_amd
    rng = np.random.default_rng(5)
    pk = np.zeros((n_windows, n_pairs), dtype=tdoa_amd.capi.PEAK_DTYPE)
    pk["lag"] = rng.integers(-20000, 20001, pk.shape)
    pk["abs_corr"] = rng.random(pk.shape)
    pk["corr"] = rng.standard_normal(pk.shape)
    return pk


def test_dump_outputs_writes_the_peak_records_as_float_arrays(tmp_path):
    import numpy as np
    pk = _peaks(99, 3)
    fixes = [(0, (41.2, -96.0, 400.0), 6, np.array([1.0, -2.0, 3.0]), None)]
    names = bench.dump_outputs(str(tmp_path / "out"), pk, fixes)
    assert names == ["peak_abs_corr", "peak_corr", "peak_lag", "solve_lat_lon", "solve_median_target_lags", "solve_status"]
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["peak_lag"], pk["lag"]) and np.array_equal(got["peak_abs_corr"], pk["abs_corr"])
    assert np.array_equal(got["peak_corr"], pk["corr"])
    assert got["solve_lat_lon"].tolist() == [[41.2, -96.0]] and got["solve_median_target_lags"].tolist() == [[1.0, -2.0, 3.0]]
    assert bench.dump_outputs(str(tmp_path / "single"), pk, []) == ["peak_abs_corr", "peak_corr", "peak_lag"]


def test_dump_outputs_past_the_limit_is_a_fixed_sample_of_windows(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20 * 3 * 100)
    pk = _peaks(1000, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), pk, [])
    sizes = sum(np.load(p).nbytes for p in (tmp_path / "a").iterdir())
    assert sizes <= bench.DUMP_LIMIT_BYTES
    rows = np.load(tmp_path / "a" / "peak_window_index.npy").astype(int)
    assert len(rows) > 50 and np.array_equal(rows, np.load(tmp_path / "b" / "peak_window_index.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "peak_corr.npy"), pk["corr"][rows])


def test_full_is_off_by_default():
    """a plain run times the steps and prints the line; the extra legs only run with --full, which the --no-* switches thin"""
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and plain.steps == 20 and plain.warmup == 5
    full = bench.parse_args(["--full", "--no-cpu-baseline", "--no-h2d"])
    assert full.full and full.no_cpu_baseline and full.no_h2d and not full.no_graph_leg and not full.no_clocks


def test_scripts_that_read_the_full_fields_ask_for_them():
    """fields a plain run no longer prints: a bench.py call of a script that reads one of them passes --full (a call piped
    into a reader on its own line is judged by that line, any other by its whole script)"""
    import glob
    import re
    full_only = ("roofline", "kernels_ms_per_step", "graph_replay", "parity_window0", "cpu_baseline", "end_to_end_h2d",
                 "sharded_cfg4", "dominant_chosen_by")

    def reads_full(text):
        return any(re.search(r"\b%s\b" % k, text) for k in full_only)

    checked = 0
    for f in sorted(glob.glob(os.path.join(ROOT, "scripts", "*.sh"))):
        text = open(f).read()
        for ln in text.splitlines():
            if not re.search(r"python3? bench\.py", ln) or ln.lstrip().startswith("#"):
                continue
            if reads_full(ln if "sys.stdin" in ln else text):
                assert "--full" in ln, "%s: %s" % (os.path.basename(f), ln.strip())
                checked += 1
    assert checked > 0


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout == ""
