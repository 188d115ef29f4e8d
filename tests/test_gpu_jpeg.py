"""GPU tier of the JPEG decoder: the case bodies of tests/jpeg_cases.py on the device (libodtk.so's kernels of csrc/jpeg.hip)."""
import os

import numpy as np
import pytest

import jpeg_cases as JC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', JC.DECODABLE)
def test_decode_against_pil(name, dev):
    JC.check_fixture(name, dev)


@pytest.mark.parametrize('order', [[0, 1, 2, 3], [3, 1, 0, 2]])
def test_mixed_batch_equals_single_decodes(order, dev):
    JC.check_mixed_batch(dev, order)


@pytest.mark.parametrize('name', ['s444_24x40', 's420_37x51'])
def test_device_equals_the_emulation_byte_for_byte(name, dev):
    """the float path is fixed by the contract in include/odtk.h (sums in index order, no fused multiply-add, rint): the device gives the bytes the CPU
    emulation of the same source gave (tests/golden/jpeg/<name>.emu.npy, kept current by tests/test_cpu_jpeg.py)"""
    got = JC.decode_batch([JC.fixture_bytes(name)], dev)[0]
    want = np.load(os.path.join(JC.GOLDEN, name + '.emu.npy'))
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f'{name}: {int((diff != 0).sum())} of {diff.size} bytes differ, max {int(diff.max())}')
    assert np.array_equal(got, want)


def test_33_copies_cross_the_prefix_table(dev):
    JC.check_many_copies(dev)


def test_decoder_reuse_with_a_smaller_second_batch(dev):
    JC.check_decoder_reuse(dev)
