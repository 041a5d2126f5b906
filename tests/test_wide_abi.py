"""The wide Behler route's interface without a GPU (include/annp_hip.h, annp_hip_eval_path 6): the two new entry points are exported,
bound and declared, the ABI version did not move, the shape check of annp_hip_init lets the larger Behler shapes through to the device
check (and still refuses what lies beyond, and every oversized Chebyshev file), and the host parser carries a 16 + 48 file."""
import os
import subprocess

import numpy as np
import pytest

from annp_testlib import read_pot, write_ann

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ABI = ["annp_hip_descriptor_pitch", "annp_hip_last_descriptors_pitched"]
RC = 7.3699319


def behler_set(npsf, ntsf):
    rad = [(0.004 + 0.003 * m, 0.0, RC) for m in range(npsf)]
    ang = [(0.003 + 0.002 * (m % 5), -1.0 if m % 2 else 1.0, float(1 + m % 6), RC) for m in range(ntsf)]
    return rad, ang


@pytest.fixture(scope="module")
def lib():
    from meng_zhang_amd.lib import load_library
    return load_library()


def test_library_exports_the_entry_points():
    so = os.path.join(ROOT, "meng_zhang_amd", "libannp_hip.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for name in NEW_ABI:
        assert (" T " + name + "\n") in syms, name


def test_binding_header_and_abi_version(lib):
    from meng_zhang_amd.lib import ABI_SYMBOLS, ABI_VERSION
    for name in NEW_ABI:
        assert name in ABI_SYMBOLS and getattr(lib, name).argtypes is not None
    assert ABI_VERSION == 7 and lib.annp_hip_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "annp_hip.h")).read()
    assert "#define ANNP_HIP_ABI_VERSION 7" in header
    assert "int annp_hip_descriptor_pitch(const annp_hip_handle *handle);" in header
    assert "int annp_hip_last_descriptors_pitched(annp_hip_handle *handle, double *rows, int inum, int pitch);" in header
    assert " *   6  Behler G2/G4, the wide kernels" in header
    assert lib.annp_hip_descriptor_pitch(None) == -1 and lib.annp_hip_last_descriptors_pitched(None, None, 0, 64) == -1


def _init_code(path, elem):
    from meng_zhang_amd import PairANNP
    p = PairANNP(ntypes=1, device=0)
    try:
        p.settings([])
        p.coeff(["*", "*", path, elem])
        with pytest.raises(RuntimeError) as err:
            p.init_style()
        return str(err.value)
    finally:
        p.close()


def test_shape_check_by_descriptor_without_a_gpu(tmp_path):
    """annp_hip_init checks the shape before it looks for a device: a Behler file the wide kernels take now fails with -4 on a box
    without a GPU (it failed with -9 before the route existed), what lies beyond their limits and every oversized Chebyshev file with -9"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    net = dict(ntl=4, acts=("ta", "ta", "li"), seed=3, element="Ni")
    accepted = {"nsf40": dict(nnod=12, behler=behler_set(12, 28)), "nnod48": dict(nnod=48, behler=behler_set(2, 7)),
                "npsf12": dict(nnod=12, behler=behler_set(12, 8))}
    for name, kw in accepted.items():
        msg = _init_code(write_ann(str(tmp_path / (name + ".ann")), **dict(net, **kw)), "Ni")
        assert "code -4" in msg, (name, msg)
    refused = {"nsf65": (dict(nnod=12, behler=behler_set(17, 48)), "nsf=65"), "nnod65": (dict(nnod=65, behler=behler_set(2, 7)), "nnod=65"),
               "npsf33": (dict(nnod=12, behler=behler_set(33, 8)), "npsf=33")}
    for name, (kw, text) in refused.items():
        msg = _init_code(write_ann(str(tmp_path / (name + ".ann")), **dict(net, **kw)), "Ni")
        assert "code -9" in msg and text in msg, (name, msg)
    for kw in (dict(nnod=33), dict(npsf=10, ntsf=19), dict(npsf=9, ntsf=20)):          # Chebyshev: the limits did not move
        args = dict(npsf=9, ntsf=19, nnod=10, ntl=4, acts=("ta", "ta", "li"))
        args.update(kw)
        msg = _init_code(write_ann(str(tmp_path / "cheb.ann"), **args), "Fe")
        assert "code -9" in msg, (kw, msg)


def test_host_parser_round_trips_a_16_plus_48_file(tmp_path):
    from meng_zhang_amd import PairANNP
    rad, ang = behler_set(16, 48)
    path = write_ann(str(tmp_path / "full.ann"), nnod=64, ntl=5, acts=("ta", "hy", "si", "li"), seed=5, element="Ni", behler=(rad, ang))
    o = read_pot(path)
    p = PairANNP(ntypes=1, device=0)
    try:
        p.settings([])
        p.coeff(["*", "*", path, "Ni"])
        q = p.potential()
    finally:
        p.close()
    assert (q["ntl"], q["nnod"], q["nsf"], q["npsf"], q["ntsf"], q["has_symcoef"]) == (5, 64, 64, 16, 48, 1)
    assert (o.ntl, o.nnod, o.nsf, o.npsf, o.ntsf) == (5, 64, 64, 16, 48)
    assert list(q["flagact"]) == [o.flagact[l] for l in range(4)] == [4, 1, 2, 0]
    assert np.array_equal(q["norm_a"], np.array(o.norm0[:64])) and np.array_equal(q["norm_b"], np.array(o.norm1[:64]))
    assert np.array_equal(q["sym_rad"], np.array([list(o.sym_rad[m]) for m in range(16)]))
    assert np.array_equal(q["sym_ang"], np.array([list(o.sym_ang[m]) for m in range(48)]))
    assert np.allclose(q["sym_rad"], np.array(rad), atol=1e-7) and np.allclose(q["sym_ang"], np.array(ang), atol=1e-7)
    stride = len(o.W[0]) // len(o.B[0])           # row pitch of the oracle's weight image
    for l in range(4):
        nr, nc = q["W"][l].shape
        w = np.array(o.W[l][: nr * stride]).reshape(nr, stride)[:, :nc] if stride != nc else np.array(o.W[l][: nr * nc]).reshape(nr, nc)
        assert np.array_equal(q["B"][l], np.array(o.B[l][:nr]))
        assert np.array_equal(q["W"][l], w) or np.array_equal(q["W"][l], np.array(o.W[l][: nr * nc]).reshape(nr, nc))
