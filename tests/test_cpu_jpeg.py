"""CPU tier of the JPEG decoder (include/odtk.h, "JPEG").  The host entry points (odtk_jpeg_info, odtk_jpeg_entropy_decode, odtk_jpeg_plan_init) run from
the real libodtk.so; the two kernels of csrc/jpeg.hip run from source under the fiber emulation (jpeg_cases.emulated).  Bounds: jpeg_cases' docstring."""
import concurrent.futures
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import jpeg_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _lib():
    import odtk  # noqa: F401
    from odtk import _lib
    return _lib


def _decode_host(data, capacity=None):
    """(rc, message, coef, qtables) through the real library, the coefficient buffer between guard words that must survive"""
    import ctypes as C
    L = _lib()
    lib = L.load()
    info = L.JpegInfo()
    rc = lib.odtk_jpeg_info(data, len(data), C.byref(info))
    if rc != 0:
        return rc, lib.odtk_last_error().decode(), None, None
    cap = int(info.coef_count) if capacity is None else capacity
    buf = np.full(cap + 2 * GUARD, 0x5a5a, np.int16)
    qt = np.full(256 + 2 * GUARD, 0xa5a5, np.uint16)
    rc = lib.odtk_jpeg_entropy_decode(data, len(data), buf.ctypes.data + 2 * GUARD, cap, qt.ctypes.data + 2 * GUARD)
    msg = lib.odtk_last_error().decode() if rc else ''
    assert (buf[:GUARD] == 0x5a5a).all() and (buf[GUARD + cap:] == 0x5a5a).all(), 'coefficient guard words overwritten'
    assert (qt[:GUARD] == 0xa5a5).all() and (qt[GUARD + 256:] == 0xa5a5).all(), 'table guard words overwritten'
    return rc, msg, buf[GUARD: GUARD + cap].copy(), qt[GUARD: GUARD + 256].copy()


def test_library_exports_the_jpeg_entry_points():
    L = _lib()
    lib = L.load()
    assert lib.odtk_version() >= 103
    for name in ('odtk_jpeg_info', 'odtk_jpeg_entropy_decode', 'odtk_jpeg_plan_init', 'odtk_jpeg_reconstruct'):
        assert name in L.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize('name', JC.DECODABLE)
def test_info_of_every_fixture(name):
    from odtk import ops
    e = JC.MANIFEST[name]
    i = ops.jpeg_info(JC.fixture_bytes(name))
    nc = 1 if e['mode'] == 'L' else 3
    hs, vs = e['sampling']
    assert (i.width, i.height, i.ncomp) == (e['width'], e['height'], nc)
    assert (i.hsamp[0], i.vsamp[0]) == (hs, vs) and all((i.hsamp[c], i.vsamp[c]) == (1, 1) for c in range(1, nc))
    mw, mh = -(-e['width'] // (8 * hs)), -(-e['height'] // (8 * vs))
    assert (i.mcu_w, i.mcu_h) == (mw, mh)
    blocks = [mw * hs * mh * vs] + [mw * mh] * (nc - 1)
    assert list(i.blocks)[:nc] == blocks and i.coef_count == 64 * sum(blocks)
    assert list(i.coef_offset)[:nc] == [64 * sum(blocks[:c]) for c in range(nc)]
    assert all(0 <= i.tq[c] <= 3 for c in range(nc))
    assert i.restart_interval == (2 if name.endswith('_rst') else 0)


@pytest.mark.parametrize('name', JC.DECODABLE)
def test_emulated_decode_against_pil(name):
    with JC.emulated():
        JC.check_fixture(name, 'cpu')


@pytest.mark.parametrize('order', [[0, 1, 2, 3], [3, 1, 0, 2]])
def test_emulated_mixed_batch_equals_single_decodes(order):
    with JC.emulated():
        JC.check_mixed_batch('cpu', order)


def test_emulated_many_copies_and_decoder_reuse():
    with JC.emulated():
        JC.check_many_copies('cpu')
        JC.check_decoder_reuse('cpu')


def test_emulated_fixtures_are_current():
    """tests/golden/jpeg/<name>.emu.npy (what the GPU tier compares the device with, byte for byte) is what the emulation gives today"""
    with JC.emulated():
        for name in ('s444_24x40', 's420_37x51'):
            got = JC.decode_batch([JC.fixture_bytes(name)], 'cpu')[0]
            assert np.array_equal(got, np.load(os.path.join(JC.GOLDEN, name + '.emu.npy'))), name


def test_restart_markers_are_consumed_and_required():
    data = JC.fixture_bytes('s420_64x48_rst')
    assert data.count(b'\xff\xd0') >= 1 and _decode_host(data)[0] == 0
    at = data.index(b'\xff\xd0')
    rc, msg, _, _ = _decode_host(data[:at] + b'\x12\x34' + data[at + 2:])          # the first restart marker overwritten with entropy bytes
    assert rc != 0 and msg
    from odtk import ops
    assert ops.jpeg_info(data).restart_interval == 2


def test_16_bit_tables_and_tables_of_ones_reach_the_decoder():
    rc, _, coef, qt = _decode_host(JC.fixture_bytes('s420_40x24_q16bit'))
    assert rc == 0 and int(qt.max()) > 255
    rc, _, coef, qt = _decode_host(JC.fixture_bytes('s420_40x24_q100'))
    assert rc == 0 and (qt[:128] == 1).all() and int(np.abs(coef).max()) > 255          # tables of ones: the largest coefficient range


@pytest.mark.parametrize('name,word', [('progressive_24x24', 'progressive'), ('cmyk_16x16', 'CMYK'), ('rgb_16x16', 'RGB-coded')])
def test_unsupported_files_are_refused_with_a_message(name, word):
    from odtk import ops
    rc, msg, _, _ = _decode_host(JC.fixture_bytes(name))
    assert rc != 0 and word in msg and 'not supported' in msg
    with pytest.raises(_lib().OdtkError, match=word):
        ops.jpeg_info(JC.fixture_bytes(name))


def test_rgb_component_ids_without_jfif_are_refused():
    """libjpeg's rule for three components without a JFIF or Adobe marker: ids 'R', 'G', 'B' mean RGB.  A fixture with its APP0 segment cut out and its
    component ids rewritten (frame header and scan header) must be refused; with only the APP0 cut out (ids 1, 2, 3) it is YCbCr and decodes."""
    data = bytearray(JC.fixture_bytes('s444_24x40'))
    assert data[2:4] == b'\xff\xe0'
    n = 2 + ((data[4] << 8) | data[5])
    bare = data[:2] + data[2 + n:]
    assert _decode_host(bytes(bare))[0] == 0
    sof, sos = bare.index(b'\xff\xc0'), bare.index(b'\xff\xda')
    for c, ch in enumerate(b'RGB'):
        bare[sof + 10 + 3 * c] = ch
        bare[sos + 5 + 2 * c] = ch
    rc, msg, _, _ = _decode_host(bytes(bare))
    assert rc != 0 and 'RGB-coded' in msg


def test_capacity_too_small_is_refused():
    data = JC.fixture_bytes('s420_8x8')
    for cap in (0, 64, 383):
        rc, msg, _, _ = _decode_host(data, cap)
        assert rc != 0 and 'too small' in msg
    assert _decode_host(data, 384)[0] == 0


def test_every_truncation_of_the_smallest_fixture():
    data = JC.fixture_bytes(min(JC.DECODABLE, key=lambda n: JC.MANIFEST[n]['bytes']))
    for n in range(len(data)):
        rc, msg, _, _ = _decode_host(data[:n])
        assert rc == 0 or msg, n
    assert _decode_host(data[: len(data) // 2])[0] != 0 and _decode_host(data)[0] == 0


def test_200_seeded_corruptions():
    data = bytearray(JC.fixture_bytes('s420_37x51'))
    rng = np.random.default_rng(7)
    refused = 0
    for _ in range(200):
        at, v = int(rng.integers(len(data))), int(rng.integers(256))
        bad = bytearray(data)
        bad[at] = v if v != bad[at] else v ^ 0xff
        rc, msg, _, _ = _decode_host(bytes(bad))
        assert rc == 0 or msg
        refused += rc != 0
    assert refused > 0


def test_plan_init_rejects_inconsistent_info_and_alignment():
    import ctypes as C
    from odtk import ops
    L = _lib()
    info = ops.jpeg_info(JC.fixture_bytes('s420_37x51'))
    plan = L.JpegPlan()
    ops.jpeg_plan_init(plan, info, 4096, 8192, 16384, 32768, 5, 7)
    assert (plan.unit_start, plan.unit_count, plan.tile_start, plan.tile_count) == (5, -(-int(info.coef_count) // 1024), 7, -(-37 * 51 // 1024))
    assert list(plan.block_start) == [0, 48, 60, 72] and (plan.hs, plan.vs) == (2, 2)
    with pytest.raises(L.OdtkError, match='alignment'):
        ops.jpeg_plan_init(plan, info, 4098, 8192, 16384, 32768, 0, 0)
    info.width = 400
    with pytest.raises(L.OdtkError, match='coef_count'):
        ops.jpeg_plan_init(plan, info, 4096, 8192, 16384, 32768, 0, 0)
    assert C.sizeof(L.JpegPlan) % 8 == 0


def test_eight_threads_decode_different_fixtures_at_once():
    names = (JC.DECODABLE * 2)[:8]
    single = {n: _decode_host(JC.fixture_bytes(n)) for n in set(names)}

    def work(n):
        out = None
        for _ in range(20):
            out = _decode_host(JC.fixture_bytes(n))
        return out
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        for n, (rc, msg, coef, qt) in zip(names, pool.map(work, names)):
            assert rc == 0 and np.array_equal(coef, single[n][2]) and np.array_equal(qt, single[n][3]), n


def test_fuzz_program_under_sanitizers():
    """tests/jpeg_fuzz_host.cpp + csrc/jpeg_host.h, g++ -fsanitize=address,undefined, as a child process: truncations and corruptions, exit status 0"""
    exe = os.path.join(tempfile.mkdtemp(prefix='odtk_jpeg_fuzz_'), 'jpeg_fuzz_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-static-libasan', '-static-libubsan',          # the runtimes inside the program: nothing about it depends on load order
                           os.path.join(ROOT, 'tests', 'jpeg_fuzz_host.cpp'), '-o', exe])
    small = min(JC.DECODABLE, key=lambda n: JC.MANIFEST[n]['bytes'])
    r = subprocess.run([exe, os.path.join(JC.GOLDEN, small + '.jpg'), os.path.join(JC.GOLDEN, 's420_37x51.jpg')], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout
