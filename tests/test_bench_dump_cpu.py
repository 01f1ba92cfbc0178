"""bench.py --dump-outputs: what dump_outputs writes for the benchmarked model (deit_small W4A4, wrapped as bench.py wraps
it; calibration itself is not needed to check the format) -- one .npy per state_dict entry, float32 / float64, a fixed
seeded sample of the large entries, under 64 MB in all."""
import os

import numpy as np
import torch

import bench
from adalog_amd.utils.models import create_model
from adalog_amd.utils.wrap_net import wrap_modules_in_net


def test_dump_outputs_format(tmp_path):
    torch.manual_seed(5)
    model = wrap_modules_in_net(create_model("deit_small").eval(), bench.load_cfg(4), reparam=True)
    sd = model.state_dict()
    bench.dump_outputs(model, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(k + ".npy" for k in sd)
    assert sum(os.path.getsize(tmp_path / n) for n in names) < 64 << 20
    for key, t in sd.items():
        a = np.load(tmp_path / (key + ".npy"))
        assert a.dtype in (np.float32, np.float64)
        flat = t.reshape(-1).double()
        if t.numel() > bench.DUMP_SAMPLE:
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:bench.DUMP_SAMPLE].sort().values
            assert a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a.astype(np.float64), flat[idx].numpy())
        else:
            assert a.shape == tuple(t.shape) and np.array_equal(a.reshape(-1).astype(np.float64), flat.numpy())
