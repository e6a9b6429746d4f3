import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP device) to run")


def load_npz(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def block_fixtures():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "block_*.npz")))


def rel_to_max(a, b):
    """max|a-b| / max|b|  (the tolerance measure used throughout)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    denom = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / denom)


@pytest.fixture
def oracle_threads():
    """Runs a test with torch's CPU thread count fixed at 8: the fp32 oracle's
    summation order, and with it its rounding, follows the thread count (at odd
    counts the first BatchNorm's weight gradient moves by 3e-4 rel-to-max), so
    the tests that compare it with an fp32 fixture do not take the host's."""
    import torch
    prev = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(prev)


def fp32_pair_tol(base, err64):
    """Bound on fp32 oracle vs fp32 reference fixture for one tensor. Both are
    roundings of the same exact result, and their summation order differs with
    the CPU and its thread count, so they agree only as well as each agrees with
    exact arithmetic. ``err64`` is the fixture's own distance from the fp64
    oracle (one draw of that rounding error, same measure as the bound); either
    run is allowed twice that draw: |oracle - fixture| <= 2 err64 + 2 err64.
    Where the fixture is accurate (err64 << base) the bound stays ``base``; it
    grows only on gradients that are small differences of large terms
    (test_oracle_golden.test_stack_fp32_conditioning_is_documented)."""
    return max(base, 4.0 * err64)


@pytest.fixture(scope="session")
def pkg():
    from stgcn_loader import load
    return load()
