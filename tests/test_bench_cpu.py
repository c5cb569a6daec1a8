"""bench.py host logic that needs no GPU: the committed PMC profile must resolve for every conv kernel class of the default workload
(kernel names carry template arguments that change when a kernel gains one — the roofline's `traffic` went null that way once)."""
import argparse

import bench


def test_committed_pmc_profile_resolves_for_the_default_workload():
    """The committed PMC profile either belongs to THESE sources (then every conv kernel class of the default workload resolves in it) or
    is reported stale and contributes nothing — old bytes are never attached to new kernels."""
    import json
    import os
    args = argparse.Namespace(ver="yolov7", mode="kfiou", size=800, nc=16, batch=64)
    path = os.path.join(bench.ROOT, bench.PMC_PROFILE)
    fresh = os.path.exists(path) and json.load(open(path)).get("source_sha256") == bench.source_sha256()
    t = bench.pmc_traffic(args)
    if fresh:
        for cls in ("conv_gemm_kernel<128x128,1x1>", "conv_gemm_kernel<128x128>", "conv_gemm_kernel<256x64>", "conv3x3_patch_kernel<256x128>", "conv3x3_patch_kernel<256x64>",
                    "conv_wgrad_kernel<128>", "conv3x3_wgrad_kernel<128x9x32>"):
            assert t.get(cls, 0) > 1_000_000, (cls, t.get(cls))
        assert 150e9 < bench.pmc_step_bytes(args) < 400e9
    else:
        assert t == {} and bench.pmc_step_bytes(args) == 0
    other = argparse.Namespace(ver="yolov7", mode="kfiou", size=800, nc=16, batch=8)
    assert bench.pmc_traffic(other) == {} and bench.pmc_step_bytes(other) == 0


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: small arrays are written whole, large ones as the same seeded sample on every call; files are float32 / float64."""
    import numpy as np
    import torch
    small = torch.arange(10, dtype=torch.float32)
    assert np.array_equal(bench._sample(small, seed=1), small.numpy())
    big = torch.randn(3 * bench.DUMP_SAMPLE, generator=torch.Generator().manual_seed(0))
    a, b = bench._sample(big, seed=5), bench._sample(big.clone(), seed=5)
    assert a.dtype == np.float32 and a.size == bench.DUMP_SAMPLE and np.array_equal(a, b)
    assert not np.array_equal(a, bench._sample(big, seed=6))
    last = {"loss": torch.tensor([2.5]), "items": {"reg_loss": torch.tensor(1.0), "total_loss": 2.5},
            "outs": [torch.ones(2, 3, 4, 4, 22), big.view(-1, 16)[:1000]]}
    arrays = bench.sample_outputs(last, big)
    bench.write_outputs(str(tmp_path / "d"), arrays)
    names = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert names == ["head0.npy", "head1.npy", "loss.npy", "loss_reg_loss.npy", "loss_total_loss.npy", "params_after_step.npy"]
    assert np.load(tmp_path / "d" / "loss.npy").dtype == np.float64 and float(np.load(tmp_path / "d" / "loss_total_loss.npy")[0]) == 2.5
    assert np.array_equal(np.load(tmp_path / "d" / "params_after_step.npy"), bench._sample(big, seed=100))
