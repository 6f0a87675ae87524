"""bench.py's plain run and --dump-outputs: a plain run times the steps and nothing else (--full adds the rest), and
--dump-outputs writes what the timed path returned in its last step, exactly, as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _u64(a):
    """[high 32 bits, low 32 bits] as written by bench.summary_arrays -> the u64"""
    hi, lo = (int(x) for x in a)
    return (hi << 32) | lo


def test_plain_is_the_default_and_full_an_option():
    import bench

    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    assert bench.parse_args(["--config", "4"]).histogram == 20      # the step itself: no --full needed
    assert bench.parse_args(["--histogram", "16", "--full"]).histogram == 16


def test_extra_histogram_needs_full():
    import bench

    with pytest.raises(SystemExit):
        bench.parse_args(["--histogram", "16"])


def test_summary_arrays_are_exact(tmp_path):
    import bench

    words = np.array([0, 1, (1 << 64) - 1, 0x8000000000000001, 0x123456789ABCDEF0], dtype=np.uint64)
    fields = ["a", "b", "c", "d", "e"]
    arrs = bench.summary_arrays(words, fields, prefix="rank1_")
    assert sorted(arrs) == ["rank1_" + f for f in fields]
    bench.write_outputs(str(tmp_path / "d"), arrs)
    for f, w in zip(fields, words):
        a = np.load(tmp_path / "d" / f"rank1_{f}.npy")
        assert a.dtype == np.float64 and a.shape == (2,)
        assert _u64(a) == int(w)


def test_counts_arrays_small_and_sampled():
    import bench

    small = np.arange(1 << 10, dtype=np.uint64) * np.uint64(3)
    d = bench.counts_arrays(small)
    assert list(d) == ["counts"] and (d["counts"] == small.astype(np.float64)).all()
    big = np.arange(1 << 24, dtype=np.uint64)
    d1, d2 = bench.counts_arrays(big), bench.counts_arrays(big)
    assert sorted(d1) == ["counts_sample", "counts_sample_index"]
    assert sum(a.nbytes for a in d1.values()) <= 64 << 20
    assert all((d1[k] == d2[k]).all() for k in d1)                   # a fixed sample
    assert (d1["counts_sample"] == d1["counts_sample_index"]).all()  # values are those at the indices


def _run_plain(tmp_path, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--dump-outputs", str(d), *args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    line = json.loads(lines[0])
    # a plain run: the headline and nothing measured beside it
    assert line["full"] is False and line["steps"] == 4 and line["ms_per_step"] > 0
    for key in ("cpu_baseline", "sustained", "parity_vs_oracle"):
        assert key not in line
    assert line["roofline"]["traffic"] is None
    return line, d


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["1", "3"])
def test_plain_run_dumps_the_summary(tmp_path, orc, cfg):
    from kmers_amd.api import SEED_DEFAULT

    n, L, k = 100_000, 150, 31
    line, d = _run_plain(tmp_path, "--config", cfg, "--reads-per-gpu", str(n))
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - n * (L - k + 1)) < 1e-6 * n * (L - k + 1)
    assert sorted(os.listdir(d)) == ["n_valid.npy", "sum_canon.npy", "sum_fw.npy", "xor_hash.npy"]
    host = orc.gen_reads(SEED_DEFAULT, 0, n * L)
    o = orc.canonical_reduce(host, n, L, k, hasher_k=k if cfg == "3" else 0)
    assert _u64(np.load(d / "n_valid.npy")) == o.n_valid == n * (L - k + 1)
    assert _u64(np.load(d / "sum_canon.npy")) == o.sum_canon
    assert _u64(np.load(d / "xor_hash.npy")) == (o.xor_hash if cfg == "3" else 0)


@pytest.mark.gpu
def test_plain_run_dumps_the_two_word_summary(tmp_path, orc):
    from kmers_amd.api import SEED_DEFAULT

    n, L, k = 100_000, 150, 63
    _, d = _run_plain(tmp_path, "--config", "2", "-k", str(k), "--reads-per-gpu", str(n))
    o = orc.canonical_reduce2(orc.gen_reads(SEED_DEFAULT, 0, n * L), n, L, k, with_hash=False)
    for f in ("n_valid", "sum_lo", "sum_hi", "xor_lo", "xor_hi"):
        assert _u64(np.load(d / f"{f}.npy")) == getattr(o, f), f


@pytest.mark.gpu
def test_plain_run_dumps_the_histogram(tmp_path, orc):
    from kmers_amd.api import SEED_DEFAULT

    n, L, k = 20_000, 150, 31
    _, d = _run_plain(tmp_path, "--config", "4", "--reads-per-gpu", str(n))
    assert sorted(os.listdir(d)) == ["counts.npy"]
    got = np.load(d / "counts.npy")
    assert got.dtype == np.float64 and got.size == 1 << 20
    o = orc.histogram(orc.gen_reads(SEED_DEFAULT, 0, n * L), n, L, k, k, 20)
    assert (got == o.astype(np.float64)).all()
