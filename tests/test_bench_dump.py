"""bench.py --dump-outputs on the CPU: the limb arrays are written exactly, and an output over the size limit keeps the same
fixed, seeded rows of every array."""
import numpy as np

import bench
from pailliercryptolib_amd.limbs import limbs_to_ints


def _ints(a32):
    """float64 32-bit limbs (least significant first) -> Python ints"""
    return [sum(int(v) << (32 * i) for i, v in enumerate(row)) for row in a32]


def test_dump_is_exact(tmp_path):
    rng = np.random.default_rng(7)
    c = rng.integers(0, 2**64, size=(5, 64), dtype=np.uint64)
    m = rng.integers(0, 2**64, size=(5, 32), dtype=np.uint64)
    bench.dump_outputs(str(tmp_path), {"ciphertext": c, "plaintext": m})
    for name, a in (("ciphertext", c), ("plaintext", m)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == (a.shape[0], 2 * a.shape[1])
        assert _ints(got) == limbs_to_ints(a)
    assert not (tmp_path / "row_index.npy").exists()


def test_dump_samples_the_same_rows_when_too_large(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 1024)
    rows = 200
    a = np.arange(rows * 4, dtype=np.uint64).reshape(rows, 4) * np.uint64(0x100000001)
    b = np.arange(rows * 2, dtype=np.uint64).reshape(rows, 2)
    bench.dump_outputs(str(tmp_path / "one"), {"a": a, "b": b})
    bench.dump_outputs(str(tmp_path / "two"), {"a": a, "b": b})
    idx = np.load(tmp_path / "one" / "row_index.npy").astype(np.int64)
    keep = 8 * 1024 // ((4 + 2) * 2 * 8)
    assert len(idx) == keep < rows and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "two" / "row_index.npy"))
    ga, gb = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "one" / "b.npy")
    assert _ints(ga) == limbs_to_ints(a[idx]) and _ints(gb) == limbs_to_ints(b[idx])
    assert ga.nbytes + gb.nbytes <= 8 * 1024
