"""CPU check of the gradient's boundary: both entry points are declared in include/psoap_gp.h, bound in
psoap_amd._lib.SIGNATURES with the declared argument lists, exported by the built library, and reachable from Python."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("psoap_chunk_lnlike_grad", "psoap_chunk_grad_release")


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/psoap_gp.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_gradient_entry_points_are_declared_bound_and_exported():
    from psoap_amd import _lib, build
    L = ctypes.CDLL(build.build())
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    as_ctype = {"psoap_chunk *": vp, "int": ctypes.c_int, "double": ctypes.c_double, "const double *": dp, "double *": dp}
    for name in NAMES:
        args = _declaration(name)
        assert hasattr(L, name), f"{name} is not exported by libpsoap_gp.so"
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        # every declared parameter, by its type (the name dropped), is what ctypes passes
        declared = [as_ctype[re.sub(r"\s*\w+$", "", a).replace(" *", " *").strip()] for a in args]
        assert declared == list(argtypes), (name, args)
    assert len(_declaration("psoap_chunk_lnlike_grad")) == 10


def test_python_surface_exists():
    from psoap_amd import covariance
    from psoap_amd.chunk import ChunkHandle
    assert callable(ChunkHandle.lnlike_grad) and callable(ChunkHandle.grad_release)
    for f in ("lnlike_grad", "velocity_gradient", "optimize_GP", "optimize_GP_f"):
        assert callable(getattr(covariance, f))


def test_negative_hyperparameter_short_circuits_without_gpu():
    """-inf and NaN gradients before any device work, as ``_lnlike`` returns -inf there; l == 0 raises"""
    import numpy as np
    import pytest
    from psoap_amd import covariance
    x = np.linspace(8.5, 8.5001, 6)
    lnp, g_gp, g_lwl, g_mu = covariance.lnlike_grad([x, x], x, x, [0.2, 5.0, -0.1, 7.0])
    assert lnp == -np.inf and g_gp.shape == (4,) and g_lwl.shape == (2, 6)
    assert np.all(np.isnan(g_gp)) and np.all(np.isnan(g_lwl)) and np.isnan(g_mu)
    with pytest.raises(ZeroDivisionError):
        covariance.lnlike_grad([x], x, x, [0.2, 0.0])
    with pytest.raises(ValueError):
        covariance.lnlike_grad([x], x, x, [np.nan, 5.0])
