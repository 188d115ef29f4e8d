"""odtk_classify_eval and ClassificationEvaluator on the device (csrc/classify.hip in libodtk.so): the cases of tests/classify_cases.py -- integers equal to
the float64 restatement, loss within the derived bound, guard words round every output, pad columns of 1e30, ties against the head kernel's pred, non-finite
logits, labels outside [0, C), accumulation over launches, every refusal, one device-to-host copy per result()."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import classify_cases as CC              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('N,C,ldl,top_k', CC.SHAPES)
def test_shapes_against_float64(N, C, ldl, top_k):
    CC.check_shape(N, C, ldl, top_k, DEV)


def test_ties_and_the_head_kernels_pred():
    CC.check_ties(DEV)


def test_non_finite_logits():
    CC.check_non_finite(DEV)


def test_bad_labels():
    CC.check_bad_labels(DEV)


def test_accumulation_over_launches():
    CC.check_accumulation(DEV)


def test_refusals():
    CC.check_refusals(DEV)


def test_evaluator_one_read_back_and_reset():
    CC.check_evaluator(DEV)
