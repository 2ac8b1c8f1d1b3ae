"""CPU check of the posterior draws' boundary: the three entry points are declared in include/psoap_gp.h, bound in
psoap_amd._lib.SIGNATURES with the declared argument lists, exported by the built library and reachable from Python, and the
argument checks that need no device answer 2 with their message."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("psoap_chunk_predict_draw", "psoap_draw_normals", "psoap_draw_philox")


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "psoap_gp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/psoap_gp.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_draw_entry_points_are_declared_bound_and_exported():
    from psoap_amd import _lib, build
    L = ctypes.CDLL(build.build())
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    as_ctype = {"psoap_chunk *": vp, "int": ctypes.c_int, "double": ctypes.c_double, "const double *": dp, "double *": dp,
                "int *": ctypes.POINTER(ctypes.c_int), "unsigned long long": ctypes.c_ulonglong, "unsigned int": ctypes.c_uint}
    for name in NAMES:
        args = _declaration(name)
        assert hasattr(L, name), f"{name} is not exported by libpsoap_gp.so"
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        declared = []
        for a in args:
            if a.endswith("[4]"):                     # unsigned int out[4]
                declared.append(ctypes.POINTER(as_ctype[re.sub(r"\s*\w+\[4\]$", "", a)]))
            else:
                declared.append(as_ctype[re.sub(r"\s*\w+$", "", a).strip()])
        assert declared == list(argtypes), (name, args)
    assert len(_declaration("psoap_chunk_predict_draw")) == 7


def test_python_surface_exists():
    from psoap_amd import covariance, retrieve
    from psoap_amd.chunk import ChunkHandle
    sig = inspect.signature(ChunkHandle.predict_draw)
    assert list(sig.parameters) == ["self", "n_draws", "seed", "z", "nugget"] and sig.parameters["nugget"].default == 1e-8
    sig = inspect.signature(covariance.predict_draws)
    assert list(sig.parameters)[:11] == ["lwls", "fl", "sigma", "lwls_predict", "mus", "gp", "n_draws", "seed", "mode", "nugget",
                                         "baseline"]
    assert (sig.parameters["mode"].default, sig.parameters["nugget"].default, sig.parameters["baseline"].default) == (0, 1e-8, None)
    sig = inspect.signature(retrieve.retrieve_components)
    assert (sig.parameters["n_draws"].default, sig.parameters["seed"].default, sig.parameters["nugget"].default) == (0, None, 1e-8)


def test_argument_checks_that_need_no_device():
    from psoap_amd import _lib
    L = _lib.load()
    out = (ctypes.c_double * 4)()
    st = ctypes.c_int(0)
    assert L.psoap_chunk_predict_draw(None, 1, ctypes.c_ulonglong(1), None, 1e-8, out, ctypes.byref(st)) == 2
    assert L.psoap_last_error() == b"psoap_chunk_predict_draw: bad arguments"
    for D, n, o in ((0, 4, out), (1, 0, out), (1, 4, None), (2 ** 16, 2 ** 16, out)):
        assert L.psoap_draw_normals(0, ctypes.c_ulonglong(1), D, n, o) == 2
        assert L.psoap_last_error() == b"psoap_draw_normals: bad arguments"
    assert L.psoap_draw_philox(ctypes.c_ulonglong(1), 0, 0, None) == 2
    assert L.psoap_last_error() == b"psoap_draw_philox: bad arguments"
