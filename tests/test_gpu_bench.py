"""GPU: a plain `bench.py` run prints one headline line (launch-plan leg, the --steps / --warmup it was given, value
consistent with ms_per_step, none of the --full blocks), and --dump-outputs writes what the timed path computed in its
last step: the same loss, model output and parameter gradients as one eager step of the same seeded model on the same
seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_pkg, rel_err

pytestmark = pytest.mark.gpu


def test_plain_bench_run_times_the_given_steps_and_dumps_the_last_steps_outputs(tmp_path):
    import bench
    dump, B = tmp_path / "dump", 256
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--ramp-seconds", "0", "--batch", str(B), "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 7 and res["warmup"] == 2 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(B / (res["ms_per_step"] * 1e-3))
    assert res["config"]["mode"] == "launch plan (dss2_plan_run)" and res["legs"] == {"launch plan": "ok"}
    assert not {"roofline", "cpu_baseline", "other_configs", "scatter_add"} & set(res)      # --full only

    # the reference: one eager step of bench.py's model and batch (same seeds) in this process
    pkg = load_pkg()
    torch.manual_seed(0)
    b = pkg.synthetic.make_batch(["cigre14"], B, seed=1000)
    x, ei, ea = b["x"].cuda(), b["edge_index"].cuda(), b["edge_attr"].cuda()
    st = tuple(s.cuda() for s in b["stats"])
    model = pkg.MPN(8, 6, 2, bench.HID, bench.LAYERS, bench.KHOPS, 0.0).cuda()
    out = model(x[:, :8], ei, ea[:, :6])
    loss = pkg.gsp_wls_edge(input=x[:, :8], edge_input=ea[:, :6], output=out, x_mean=st[0], x_std=st[1], edge_mean=st[2],
                            edge_std=st[3], edge_index=ei, reg_coefs=bench.REG, num_samples=None, node_param=x[:, 8:],
                            edge_param=ea[:, 6:])
    loss.backward()
    want = {"loss": loss, "output": out, **{f"grad.{n}": q.grad for n, q in model.named_parameters()}}
    assert sorted(f[:-4] for f in os.listdir(dump)) == sorted(want)
    for name, w in want.items():
        got = np.load(dump / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(w.shape), name
        assert np.isfinite(got).all(), name
        # (a ReLU gate at a razor-edge pre-activation may fall the other way under another summation order and move a
        # weight-gradient row by ~1/N_nodes: the gradients' bound of __graft_entry__.smoke)
        tol = max(1e-4, 8.0 / x.shape[0]) if name.startswith("grad.") else 1e-5
        assert rel_err(torch.from_numpy(got), w) < tol, name
    assert float(np.load(dump / "loss.npy")) == np.float32(res["config"]["loss"])
