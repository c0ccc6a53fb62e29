"""bench.py's plain run and --dump-outputs: one JSON line with the headline figure only, exactly --steps timed steps, and the
last timed step's outputs on disk as float32 / float64 .npy files under 64 MB -- the same arrays the canonicalizer hands a caller
for the step's seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_bench_run_dumps_the_last_step(tmp_path):
    B, steps, warmup = 64, 3, 1
    out = tmp_path / "outputs"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--batch", str(B), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=540)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[key] is not None, key
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["value"] > 0 and abs(line["value"] - B * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    for extra in ("roofline", "stages", "self_check", "train", "configs", "tutorial", "cpu_baseline"):
        assert extra not in line, extra

    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(files) == {"canonicalized_images", "inverted_features", "group_index", "group_activations"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(out / (n + ".npy")) for n in files) <= 64 << 20
    pick = line["dump_outputs"]["images_sampled"]
    assert len(pick) == 32 and pick == sorted(set(pick)) and 0 <= pick[0] and pick[-1] < B
    assert files["canonicalized_images"].shape == (32, 3, 224, 224) and files["group_index"].shape == (B,)

    # the last timed step ran on batch (warmup + steps - 1) % 3 of bench.py's ring of 3, rank 0's seeds
    sys.path.insert(0, ROOT)
    import bench

    i = (warmup + steps - 1) % 3
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(i))
    f = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(1000 + i * 3))
    dev = torch.device("cuda:0")
    can = bench.build_canonicalizer(dev)
    with torch.no_grad():
        y = can(x.to(dev))
        inv = can.invert_canonicalization(f.to(dev), induced_rep_type="scalar")
    acts = can.canonicalization_info_dict["group_activations"].cpu()
    gidx = can.canonicalization_info_dict["group_index"].cpu()
    np.testing.assert_allclose(files["group_activations"], acts.numpy(), rtol=0, atol=1e-6 * acts.abs().max().item())
    # the index is compared wherever the top-2 margin is clear (bench.py's rule), the pixels wherever the index agrees
    top2 = acts.topk(2, dim=-1).values
    clear = ((top2[:, 0] - top2[:, 1]) > 1e-4 * acts.abs().max()).numpy()
    assert clear.sum() >= B // 2
    same = files["group_index"] == gidx.double().numpy()
    assert same[clear].all()
    rows = [k for k, p in enumerate(pick) if same[p]]
    np.testing.assert_allclose(files["canonicalized_images"][rows], y.cpu().numpy()[pick][rows], rtol=0, atol=1e-5)
    np.testing.assert_allclose(files["inverted_features"][rows], inv.cpu().numpy()[pick][rows], rtol=0, atol=1e-5)
