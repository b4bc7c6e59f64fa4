"""bench.py --dump-outputs: what the timed path returned, as float32 .npy files within the size limit (the writer alone, on the CPU)."""
import os

import numpy as np
import torch

import bench


def _spec(B, F, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(B, 1, F, T, generator=g), torch.randn(B, 1, F, T, generator=g))


def test_dump_writes_the_whole_output_below_the_limit(tmp_path):
    x = _spec(3, 16, 8)
    bench.dump_outputs(str(tmp_path / "d"), {"enhanced_spec": x})
    a = np.load(tmp_path / "d" / "enhanced_spec.npy")
    assert a.dtype == np.float32 and a.shape == (3, 1, 16, 8, 2)
    assert np.array_equal(a, torch.view_as_real(x).numpy())


def test_dump_keeps_a_fixed_sample_above_the_limit(tmp_path):
    x = _spec(4, 16, 8)
    per_item = 16 * 8 * 2 * 4
    bench.dump_outputs(str(tmp_path), {"enhanced_spec": x}, limit=2 * per_item + 100)      # the first two utterances
    a = np.load(tmp_path / "enhanced_spec.npy")
    assert a.shape == (2, 1, 16, 8, 2) and np.array_equal(a, torch.view_as_real(x[:2]).numpy())
    bench.dump_outputs(str(tmp_path), {"enhanced_spec": x}, limit=3 * 16 * 2 * 4)           # one utterance alone is too large: its first frames
    a = np.load(tmp_path / "enhanced_spec.npy")
    assert a.shape == (1, 1, 16, 3, 2) and np.array_equal(a, torch.view_as_real(x[:1, :, :, :3]).numpy())
    assert os.path.getsize(tmp_path / "enhanced_spec.npy") <= 3 * 16 * 2 * 4 + 128           # + the .npy header


def test_default_limit_is_64_mb():
    assert bench.DUMP_LIMIT_BYTES == 64 * 1024 * 1024
