"""pytest configuration: import paths + the `gpu` marker + MKL's reproducible code path.

`-m "not gpu"` = oracle vs golden vectors, host logic, C-ABI export check (runs anywhere).
`-m gpu`       = parity of the HIP path (through the C-ABI) against the oracle; needs an MI355X.
"""
import os
import sys

# Several CPU tests hold the oracle BITWISE to golden vectors of the reference.  torch's MKL picks its code path (vector math, BLAS) by
# host CPU, and the last bits differ between paths (e.g. an Intel and an AMD host), so the suite -- and tests/golden/make_golden.py, which
# writes the vectors -- run MKL on its conditional-numerical-reproducibility path, which gives the same bits on Intel and AMD hosts for
# what the suite compares (not for float32 sqrt: tests/test_sampler_cpu.py allows the generating host's last bit there).  Set before
# anything imports torch: MKL reads it at its first call.
os.environ["MKL_CBWR"] = "COMPATIBLE"

import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-diffusion360_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")


@pytest.fixture
def tune():
    """tune(gemm_cfg=4, ...) overrides tiling / kernel choices of the C ABI (cd360_set_tuning) for one test; every field is restored
    afterwards.  The C side reads no environment variables."""
    from cd360 import _lib
    saved = _lib.get_tuning()
    yield _lib.set_tuning
    _lib.set_tuning(**saved)
