"""bench.py command line: the result line, --steps, --full and
--dump-outputs (what the timed loop computed in its last step)."""

import json
import os

import numpy as np
import pytest
import torch

import bench

ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--grid", "16"]
NAMES = ("f", "dfdt", "state")


def run_bench(capsys, args):
    bench.main(args)
    lines = [ln for ln in capsys.readouterr().out.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


@pytest.fixture(scope="module")
def cpu_dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_cpu")
    bench.main(ARGS + ["--device", "cpu", "--dump-outputs", str(d)])
    return load(d)


def test_bench_result_line(capsys):
    d = run_bench(capsys, ARGS + ["--device", "cpu"])
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "Msites/s" and d["higher_is_better"] is True
    assert d["dtype"] == "fp64"
    assert d["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert np.isclose(d["value"], 16**3 / (d["ms_per_step"] * 1e-3) / 1e6)


def test_bench_full_flag(capsys):
    d = run_bench(capsys, ARGS + ["--device", "cpu", "--full"])
    assert d["steps"] == 2 and d["value"] > 0


def test_bench_dump_outputs(cpu_dump, tmp_path):
    out = cpu_dump
    assert out["f"].shape == out["dfdt"].shape == (2, 16, 16, 16)
    assert out["state"].shape == (len(bench.STATE_KEYS),)
    for v in out.values():
        assert v.dtype == np.float64 and np.isfinite(v).all()
    # the fields moved away from their initial values (f0 ~ 0.193)
    assert np.abs(out["f"] - 0.1935).max() > 1e-5
    # same arguments -> same inputs -> same outputs
    bench.main(ARGS + ["--device", "cpu", "--dump-outputs", str(tmp_path)])
    again = load(tmp_path)
    for n in NAMES:
        assert np.array_equal(out[n], again[n]), n


def test_bench_dump_steps_matter(cpu_dump, tmp_path):
    """--steps really sets the number of steps taken."""
    args = list(ARGS)
    args[args.index("--steps") + 1] = "3"
    bench.main(args + ["--device", "cpu", "--dump-outputs", str(tmp_path)])
    more = load(tmp_path)
    assert not np.array_equal(more["f"], cpu_dump["f"])
    assert more["state"][0] > cpu_dump["state"][0]      # a grows


def test_bench_dump_sampled(cpu_dump, tmp_path, monkeypatch):
    """Above the byte budget every array is sampled at the same fixed
    seeded sites: the sample is a subset of the full dump."""
    nsample = 500
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 4 * nsample)
    bench.main(ARGS + ["--device", "cpu", "--dump-outputs", str(tmp_path)])
    out = load(tmp_path)
    assert out["f"].shape == out["dfdt"].shape == (2, nsample)
    rng = np.random.default_rng(20240917)
    flat = np.sort(rng.integers(0, 16**3, size=nsample))
    for n in ("f", "dfdt"):
        assert np.array_equal(out[n], cpu_dump[n].reshape(2, -1)[:, flat])
    assert np.array_equal(out["state"], cpu_dump["state"])


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_bench_dump_outputs_gpu(cpu_dump, tmp_path):
    """The production device-resident loop dumps the same evolved
    fields as the host loop on CPU.  Tolerance: both integrate the
    same fp64 scheme for 3 steps (~1e3 flops per site and the energy
    sums over 4096 sites differ in summation order), so the results
    agree to a few 1e3 * 2**-53 relative; 1e-11 leaves a decade of
    margin."""
    bench.main(ARGS + ["--dump-outputs", str(tmp_path)])
    out = load(tmp_path)
    for n in NAMES:
        assert out[n].shape == cpu_dump[n].shape
        assert np.allclose(out[n], cpu_dump[n], rtol=1e-11, atol=1e-13), (
            n, np.abs(out[n] - cpu_dump[n]).max())
