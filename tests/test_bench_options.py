"""bench.py's command line without a GPU: the defaults of a plain run (--full off, no dump), --full and --dump-outputs
reaching the job, the combinations refused before any job starts, and dump_outputs writing the documented arrays (on a
small CPU model).  That a plain run's result line holds no --full record is checked on the GPU (test_gpu_bench.py)."""
import os

import numpy as np
import pytest
import torch

import bench


def _cfg_of(argv):
    seen = {}

    def job(cfg):
        seen["bench"] = cfg.BENCH
        return 0
    assert bench.main(argv, job=job) == 0
    return seen["bench"]


def test_plain_run_defaults():
    a = _cfg_of(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs_reach_the_job(tmp_path):
    a = _cfg_of(["--steps", "1", "--warmup", "0", "--full", "--dump-outputs", str(tmp_path / "out")])
    assert a.full is True and a.dump_outputs == str(tmp_path / "out")


@pytest.mark.parametrize("argv", [["--workload", "steve"], ["--workload", "hr"], ["--gemm-shapes"], ["--steps", "0"],
                                  ["--warmup", "-1"], ["--full", "--workload", "steve", "--dump-outputs", "x"]])
def test_refused_combinations_never_start_the_job(argv):
    def job(cfg):
        raise AssertionError("the job must not start")
    with pytest.raises(SystemExit):
        bench.main(argv, job=job)


def test_dump_outputs_writes_the_documented_arrays(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(80, 70), torch.nn.Linear(70, 5))
    unused = torch.nn.Linear(3, 3)                      # a parameter without .grad
    model.add_module("unused", unused)
    preds = model[1](model[0](torch.randn(4, 80)))
    loss = preds.square().mean()
    loss.backward()
    out = tmp_path / "d"
    bench.dump_outputs(str(out), model, preds, loss)
    got = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert set(got) == {"logits", "loss", "params_sample", "grads_sample"}
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["logits"], preds.detach().numpy())
    assert got["loss"].shape == (1,) and got["loss"][0] == np.float32(loss.item())
    # 80*70 > DUMP_SAMPLE elements: sampled; every smaller tensor whole
    n = bench.DUMP_SAMPLE + 70 + 70 * 5 + 5 + 9 + 3
    assert got["params_sample"].shape == got["grads_sample"].shape == (n,)
    np.testing.assert_array_equal(got["params_sample"][bench.DUMP_SAMPLE:bench.DUMP_SAMPLE + 70], model[0].bias.detach().numpy())
    np.testing.assert_array_equal(got["grads_sample"][bench.DUMP_SAMPLE:bench.DUMP_SAMPLE + 70], model[0].bias.grad.numpy())
    assert np.isnan(got["grads_sample"][-12:]).all() and np.isfinite(got["grads_sample"][:-12]).all()
    w = model[0].weight.detach().reshape(-1).numpy()
    assert np.isin(got["params_sample"][:bench.DUMP_SAMPLE], w).all()
    # the same positions on every run
    bench.dump_outputs(str(tmp_path / "e"), model, preds, loss)
    for name, a in got.items():
        np.testing.assert_array_equal(a, np.load(str(tmp_path / "e" / (name + ".npy"))))
