"""GPU: bench.py --dump-outputs writes what the timed path computed in its last step -- the same arrays from run to run and
whatever the number of steps, and layer 0's arrays agree with the CPU oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import cf_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, PAGE, LAYERS = 512, 16, 4
NAMES = ("out", "residual_out", "k_new", "v_new")


def _bench(dump_dir, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--seq", str(S),
                        "--page-size", str(PAGE), "--layers", str(LAYERS), "--no-configs", "--no-cpu-baseline",
                        "--dump-outputs", str(dump_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0
    return {n: np.load(os.path.join(dump_dir, n + ".npy")) for n in NAMES}


def test_bench_dump_outputs_are_the_timed_paths_results(tmp_path):
    a = _bench(tmp_path / "a", 3, 1)
    b = _bench(tmp_path / "b", 2, 2)
    for n in NAMES:
        assert a[n].dtype == np.float32 and a[n].shape == (LAYERS, 4096) and np.isfinite(a[n]).all(), n
        assert np.array_equal(a[n], b[n]), n

    # layer 0's inputs, drawn by bench.build_layers from the same seed, through the oracle
    import bench
    cap, new_kv = {}, []

    def prepare(x, res, w_qkv, w_o, kc, vc, rms_w, eps, cos, sin, **kw):
        cap.update(x=x, res=res, w_qkv=w_qkv, w_o=w_o, kc=kc, vc=vc, rms_w=rms_w, cos_sin=cos, **kw)
        return types.SimpleNamespace(outputs=(kw["out"], kw["residual_out"], None, None))
    bench.build_layers(types.SimpleNamespace(prepare_decoder_layer=prepare), torch.device("cuda:0"), 1, 0, 1, S, PAGE, new_kv=new_kv)
    c = {k: v.cpu() for k, v in cap.items() if isinstance(v, torch.Tensor)}
    ro, rr, kc, vc = O.decoder_layer_paged_batch(c["x"], c["res"], c["w_qkv"], c["w_o"], c["kv_indptr"], c["kv_indices"], c["kc"],
                                                 c["vc"], c["rms_w"], 1e-6, c["positions"], c["cos_sin"].view(-1, 128), page_size=PAGE)
    row = new_kv[0][2]
    assert np.array_equal(a["residual_out"][0], rr[0].float().numpy())
    assert np.abs(a["out"][0] - ro[0].float().numpy()).max() < 1e-3
    assert np.abs(a["k_new"][0] - kc[row].float().numpy()).max() < 2e-3
    assert np.abs(a["v_new"][0] - vc[row].float().numpy()).max() < 2e-3
