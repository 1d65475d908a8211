"""The C-ABI of the device point locator (sns_locate_points / sns_eval_p1, csrc/sns_locate.hip) without a GPU: both entry
points exist, and the argument checks that come before any device work refuse what include/sns.h says they refuse."""
import ctypes as C

import numpy as np
import pytest

from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP, mesh as M


def _locate(lib, n_nodes=4, n_tets=1, n_query=1, padding=1e-6):
    n = C.c_int64(-7)
    rc = lib.sns_locate_points(n_nodes, n_tets, None, None, n_query, None, padding, None, None, C.byref(n), None)
    return rc, n.value


def test_locate_and_eval_are_declared_and_exported(built_lib):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    for name in ("sns_locate_points", "sns_eval_p1"):
        assert name in _lib.SYMBOLS
        assert hasattr(built_lib, name)


def test_locate_refusals(built_lib):
    lib = built_lib
    assert _locate(lib, n_tets=0)[0] == -4                          # SNS_E_MESH: no tets
    assert _locate(lib, n_tets=0, n_query=0)[0] == -4
    assert _locate(lib, padding=-1e-6)[0] == -1                     # SNS_E_ARG: negative padding
    assert _locate(lib, padding=float("nan"))[0] == -1
    assert _locate(lib, n_tets=-1)[0] == -1
    assert _locate(lib, n_query=-1)[0] == -1
    assert _locate(lib, n_tets=2 ** 31)[0] == -1
    assert "padding" in lib.sns_last_error().decode()
    assert _locate(lib, n_query=0) == (0, 0)                        # no-op: SNS_OK, nothing missed, no device touched


@pytest.mark.parametrize("ncomp", [0, 5, -1])
def test_eval_refuses_ncomp_outside_1_to_4(built_lib, ncomp):
    assert built_lib.sns_eval_p1(1, None, ncomp, None, 1, None, None, None, None) == -1


def test_eval_refusals_and_noop(built_lib):
    lib = built_lib
    assert lib.sns_eval_p1(0, None, 4, None, 1, None, None, None, None) == -4       # SNS_E_MESH
    assert lib.sns_eval_p1(-1, None, 4, None, 1, None, None, None, None) == -1
    assert lib.sns_eval_p1(1, None, 4, None, -1, None, None, None, None) == -1
    for ncomp in (1, 2, 3, 4):
        assert lib.sns_eval_p1(1, None, ncomp, None, 0, None, None, None, None) == 0


def test_host_path_is_the_default_and_the_device_path_needs_a_hip_device():
    """locate_points without ``device`` is the host function as before; a CPU device is refused, not served by a fallback."""
    m = M.duct_mesh((4, 2, 2), 2.0, jitter=0.1)
    rng = np.random.default_rng(0)
    q = rng.uniform((0.1, -0.4, -0.4), (1.9, 0.4, 0.4), (50, 3))
    t, lam = IP.locate_points(m, q)
    assert t.dtype == np.int64 and lam.shape == (50, 4)
    assert np.allclose(np.einsum("na,nad->nd", lam, m.points[m.tets[t]]), q, atol=1e-12)
    with pytest.raises(ValueError, match="HIP device"):
        IP.locate_points(m, q, device="cpu")
    with pytest.raises(ValueError, match="values must be"):
        IP.eval_points(m, np.zeros((m.num_nodes, 5)), q, "cpu")
