import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    path = os.path.join(ROOT, "tests", "golden", "golden_v1.npz")
    return dict(np.load(path))


@pytest.fixture
def sock_dir(tmp_path):
    """A directory for Unix sockets: tmp_path, or a fresh short one under /tmp when tmp_path is too long for a socket
    address (sun_path holds 108 bytes, the socket's file name included)."""
    if len(os.fsencode(str(tmp_path))) <= 64:
        yield tmp_path
        return
    import shutil
    import tempfile
    from pathlib import Path
    d = tempfile.mkdtemp(prefix="psoap-", dir="/tmp")
    try:
        yield Path(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def oracle():
    """The CPU oracle (test infrastructure).  Never imported by the product."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as _oracle
    _oracle.build()
    return _oracle
