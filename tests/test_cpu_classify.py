"""CPU tier of the classification metrics: csrc/classify.hip run FROM SOURCE under the fiber emulation (tests/hip_cpu_backend.py) through the case bodies of
the GPU tier (tests/classify_cases.py: the float64 restatement, the derivation of the loss bound, the cases).  hip_cpu_backend.KERNEL_FILES is extended
for the duration of a test only and put back afterwards, as tests/test_cpu_batched_inference.py does: the coverage report of tests/test_hip_cpu.py counts on
the plain file list."""
import contextlib
import os
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import classify_cases as CC              # noqa: E402
import hip_cpu_backend as HC             # noqa: E402


@contextlib.contextmanager
def emulated():
    """the emulation with csrc/classify.hip in the build (a build of its own, cached in a directory of its own); hip_cpu_backend's module state is put back"""
    files, lib, tmp = list(HC.KERNEL_FILES), HC._LIB, tempfile.tempdir
    HC.KERNEL_FILES = files + ['classify.hip']
    HC._LIB = None
    tempfile.tempdir = os.path.join(tempfile.gettempdir(), f'odtk_cpu_classify_{os.getuid()}')
    os.makedirs(tempfile.tempdir, exist_ok=True)
    try:
        with HC.installed() as names:
            assert 'odtk_classify_eval' in names and 'odtk_gap_softmax_ce_fwd' in names
            yield
    finally:
        HC.KERNEL_FILES, HC._LIB, tempfile.tempdir = files, lib, tmp


@pytest.mark.parametrize('N,C,ldl,top_k', CC.SHAPES)
def test_emulated_shapes_against_float64(N, C, ldl, top_k):
    with emulated():
        CC.check_shape(N, C, ldl, top_k, 'cpu')


def test_emulated_ties_and_the_head_kernels_pred():
    with emulated():
        CC.check_ties('cpu')


def test_emulated_non_finite_logits():
    with emulated():
        CC.check_non_finite('cpu')


def test_emulated_bad_labels():
    with emulated():
        CC.check_bad_labels('cpu')


def test_emulated_accumulation():
    with emulated():
        CC.check_accumulation('cpu')


def test_emulated_refusals():
    with emulated():
        CC.check_refusals('cpu')


def test_emulated_evaluator():
    with emulated():
        CC.check_evaluator('cpu')


def test_module_state_is_put_back():
    files = list(HC.KERNEL_FILES)
    with emulated():
        assert HC.KERNEL_FILES[-1] == 'classify.hip'
    assert HC.KERNEL_FILES == files and 'classify.hip' not in files
