"""CPU checks of the joint predictive ABI (gphip_predict_cov / _draws / _logpdf): symbols, and argument validation that
happens before any device work."""
import ctypes

import numpy as np
import pytest

from bayesianinference_amd import _lib, build

NAMES = ("gphip_predict_cov", "gphip_predict_draws", "gphip_predict_logpdf")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_joint_symbols_are_declared_and_exported(lib):
    names = _lib.declared_symbols()
    for name in NAMES:
        assert name in names and name in _lib._SIGNATURES
        assert hasattr(lib, name)


def test_null_handle_and_null_arguments_are_rejected(lib):
    X = np.zeros((3, 1))
    out = np.zeros(9)
    info = ctypes.c_int(-1)
    dp = ctypes.POINTER(ctypes.c_double)
    o = out.ctypes.data_as(dp)
    assert lib.gphip_predict_cov(None, X.ctypes.data, 3, 0, o, o) == 1
    assert lib.gphip_predict_draws(None, X.ctypes.data, 3, 1, 2, 0, None, -1.0, o, ctypes.byref(info)) == 1
    assert lib.gphip_predict_logpdf(None, X.ctypes.data, 3, o, o, ctypes.byref(info)) == 1
    assert lib.gphip_predict_cov(None, None, 3, 0, None, None) == 1
    assert info.value == -1                        # nothing written


def _shell(lib, d=2):
    """A Handle without a device handle behind it: what the Python layer checks before it calls the library."""
    h = object.__new__(_lib.Handle)
    h._lib, h._h, h.d, h.N, h.p = lib, None, d, 5, d + 2
    return h


def test_python_layer_validates_shapes_before_device_work(lib):
    h = _shell(lib)
    with pytest.raises(_lib.GphipError) as e:
        h.predict_cov(np.zeros((0, 2)))
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.predict_cov(np.zeros((4, 3)))
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.predict_draws(np.zeros((4, 2)), 3, z=np.zeros((3, 5)))
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.predict_draws(np.zeros((4, 2)), 3, z=np.zeros((4, 3)))
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.predict_draws(np.zeros((4, 2)), 0)
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.predict_draws(np.zeros((4, 2)), 2, jitter=float("nan"))
    assert e.value.status == 1
    with pytest.raises(_lib.GphipError) as e:
        h.predict_logpdf(np.zeros((4, 2)), np.zeros(3))
    assert e.value.status == 2
