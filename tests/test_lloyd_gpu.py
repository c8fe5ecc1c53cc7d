"""The cases of tests/test_lloyd_host.py on the GPU, the float64 restatement still on the host: there the distance step is a
float32 GEMM of the vendor BLAS and the M-step an ``index_add_`` of atomics in any order.  The bounds are the ones derived in
that file's docstring, asserted as derived: a GEMM that does not keep float32 accumulation, or sums that lose more than their
n_c u, would be a finding about the distance step and not a reason to widen them."""
import numpy as np
import pytest

from . import test_lloyd_host as host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("off", host.OFFSETS)
@pytest.mark.parametrize("dim,seed", host.TRAJ)
def test_trajectory(dim, seed, off):
    """... and a second run gives the same labels in the same number of steps: atomics may move the centres by ulps, the
    margin the case asserts is what makes this a fair demand"""
    first = host.check_trajectory(DEV, dim, seed, off)
    X, init, _ = host.blobs(dim, seed, off)
    again = host.run_lloyd(DEV, X, init, tol=0.0)
    assert again[3] == first[3] and np.array_equal(again[0], first[0])


@pytest.mark.parametrize("dim,seed", host.TRAJ)
def test_translation(dim, seed):
    host.check_translation(DEV, dim, seed)


@pytest.mark.parametrize("off", [0, 30])
@pytest.mark.parametrize("dim,seed", host.TRAJ)
def test_weights_are_repetitions(dim, seed, off):
    host.check_weights_are_repetitions(DEV, dim, seed, off)


@pytest.mark.parametrize("k", [40, 100])
def test_gaussian_rows(k):
    host.check_gaussian(DEV, k)


def test_small_shapes():
    host.check_small_shapes(DEV)


def test_duplicates():
    host.check_duplicates(DEV)


def test_relocation():
    host.check_relocation(DEV)


@pytest.mark.parametrize("off", [0, 30])
def test_reducer_one_round(off):
    host.check_one_round(DEV, off)


@pytest.mark.parametrize("off", [0, 30])
def test_reducer_many_rounds(off):
    host.check_many_rounds(DEV, off)


def test_reducer_refusals():
    host.check_reducer_refusals(DEV)


@pytest.mark.parametrize("off", [30, 100])
def test_skeleton_off_centre(off):
    host.check_skeleton(DEV, off)


def test_seeding():
    host.check_seeding(DEV)


def test_predict_equals_labels_off_centre():
    host.check_predict(DEV)
