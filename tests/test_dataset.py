"""Data.dataset drop-in and the h5py-free HDF5 reader (feanet_amd.h5lite).

Checked against the reference's own data files, stored under tests/golden/ cut down to their leading samples
(tests/golden/make_h5_golden.py: h5py's own bytes, only the sample counts and the addresses behind the dropped
samples patched; the TestPoisson file is whole): every dataset's shape, and the values against raw reads at the
files' data offsets (they hold contiguous little-endian float64 blocks), plus the IsoPoisson sample the golden
fixtures were made from."""
import os

import numpy as np
import pytest
import torch

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ISO, TEST, RHS = "isopoisson_33x33_first10.h5", "testpoisson_33x33.h5", "rhs_17x17_first100_40.h5"


def raw(path, off, shape):
    return np.fromfile(os.path.join(REF, path), dtype="<f8", count=int(np.prod(shape)), offset=off).reshape(shape)


def test_h5lite_reads_reference_files(gold):
    from feanet_amd.h5lite import File
    with File(os.path.join(REF, ISO)) as h:
        assert sorted(h.keys()) == ["boundary_index", "boundary_value", "rhs", "u"]
        g = gold("datasets.npz")  # raw blocks of the uncut file (make_golden.py): the cut moved no sample
        for name in h.keys():
            np.testing.assert_array_equal(np.array(h[name])[:5], g[f"iso_{name}"])
        for name, off in (("boundary_index", 2048), ("boundary_value", 89168), ("rhs", 176288),
                          ("u", 265456)):  # u lies behind a second metadata block (2048 bytes at 263408)
            assert h[name].shape == (10, 33, 33)
            np.testing.assert_array_equal(np.array(h[name]), raw(ISO, off, (10, 33, 33)))
    with File(os.path.join(REF, TEST)) as h:
        assert h["material"].shape == (10, 32, 32, 1) and h["solution"].shape == (10, 33, 33)
        np.testing.assert_array_equal(np.array(h["dirich_idx"])[..., 0],
                                      raw(TEST, 2048, (10, 33, 33)))
        np.testing.assert_array_equal(np.array(h["solution"]), raw(TEST, 521616, (10, 33, 33)))
    with File(os.path.join(REF, RHS)) as h:
        assert h["train"].shape == (100, 17, 17) and h["test"].shape == (40, 17, 17)
        np.testing.assert_array_equal(np.array(h["train"]), raw(RHS, 2048, (100, 17, 17)))
        np.testing.assert_array_equal(np.array(h["test"]), raw(RHS, 233248, (40, 17, 17)))
        with pytest.raises(KeyError):
            h["nope"]


def test_h5lite_rejects_non_hdf5(tmp_path):
    from feanet_amd.h5lite import File
    p = tmp_path / "x.h5"
    p.write_bytes(b"not hdf5" * 100)
    with pytest.raises(ValueError):
        File(str(p))


def test_datasets_match_reference_semantics(gold):
    from Data.dataset import IsoPoissonDataSet, IsoPoissonPBCDataSet, RHSDataSet, TestPoissonDataSet
    iso = IsoPoissonDataSet(os.path.join(REF, ISO))
    assert len(iso) == 10
    u, f, bcv, bci = iso[0]
    assert u.shape == (1, 33, 33) and u.dtype == torch.float32
    np.testing.assert_array_equal(f.numpy()[0], raw(ISO, 176288, (10, 33, 33))[0].astype(np.float32))
    g = gold("mg_test_isopoisson33.npz")  # the fixtures the golden runs were made from
    np.testing.assert_array_equal(bcv.numpy()[0], g["boundary_value"][0].astype(np.float32))
    pbc = IsoPoissonPBCDataSet(os.path.join(REF, ISO))
    assert len(pbc) == 10 and torch.equal(pbc[3], iso[3][1])
    tp = TestPoissonDataSet(os.path.join(REF, TEST))
    items = tp[2]
    assert len(tp) == 10 and len(items) == 7 and all(t.dtype == torch.float64 for t in items)
    assert items[4].shape == (1, 32, 32) and items[0].shape == (1, 33, 33) and items[6].shape == (1, 33, 33)
    rhs = RHSDataSet(os.path.join(REF, RHS), case="test")
    assert len(rhs) == 40 and rhs[0].shape == (1, 17, 17)
    loader = torch.utils.data.DataLoader(iso, batch_size=8)
    ub, fb, _, _ = next(iter(loader))
    assert ub.shape == (8, 1, 33, 33)
    t2 = IsoPoissonDataSet(os.path.join(REF, ISO), transform=lambda t: 2 * t)
    assert torch.equal(t2[1][1], 2 * iso[1][1])
