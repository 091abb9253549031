"""igan_filter_images_grouped: everything is checked before any device work, so the refusals need no device.

Fake addresses stand for the buffers: a call that is refused never reads them."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W0, OUT0 = 0x10000000, 0x40000000       # 16-byte aligned, far apart


def _lib():
    from inclusivegan_amd import _abi
    lib = _abi.get_plugin()
    if lib.igan_conv_piece_form() != 2:
        pytest.skip('the grouped filter image belongs to the two-piece fp16 form (the default)')
    return _abi, lib


def _descs(_abi, entries):
    arr = (_abi.FilterImageDesc * len(entries))()
    for d, (w, out, kh, kw, cin, cout, wt) in zip(arr, entries):
        d.w, d.out, d.KH, d.KW, d.Cin, d.Cout, d.w_transposed = w, out, kh, kw, cin, cout, wt
    return arr


def _spaced(lib, n, geom=(3, 3, 128, 128)):
    step = (int(lib.igan_filter_image_bytes(*geom)) + 255) // 256 * 256
    return [(W0, OUT0 + i * step) + geom + (i & 1,) for i in range(n)]


def test_binding_matches_header():
    from inclusivegan_amd import _abi
    text = open(os.path.join(ROOT, 'include', 'igan_hip.h')).read()
    mx = int(re.search(r'#define IGAN_FILTER_MAX_GROUPS (\d+)', text).group(1))
    assert mx >= 48 and _abi.FILTER_MAX_GROUPS == mx
    body = re.search(r'typedef struct igan_filter_image_desc \{(.*?)\} igan_filter_image_desc;', text, flags=re.S).group(1)
    names = [re.findall(r'([A-Za-z_0-9]+)\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert names == [f[0] for f in _abi.FilterImageDesc._fields_]
    lib = _abi.get_plugin()
    assert lib.igan_struct_size(_abi.STRUCTS.index(_abi.FilterImageDesc)) == ctypes.sizeof(_abi.FilterImageDesc)


@pytest.mark.parametrize('count', ['zero', 'max_plus_one'])
def test_count_out_of_range(count):
    _abi, lib = _lib()
    n = 0 if count == 'zero' else _abi.FILTER_MAX_GROUPS + 1
    arr = _descs(_abi, _spaced(lib, max(n, 1)))
    assert lib.igan_filter_images_grouped(None, arr, n) == 1        # IGAN_ERR_INVALID_ARGUMENT
    assert b'count <= %d' % _abi.FILTER_MAX_GROUPS in lib.igan_last_error()


def test_null_table():
    _abi, lib = _lib()
    assert lib.igan_filter_images_grouped(None, None, 1) == 1


@pytest.mark.parametrize('geom', [(1, 1, 128, 128), (3, 3, 64, 64)], ids=['1x1', '3x3x64x64'])
def test_entry_the_library_takes_no_image_for(geom):
    _abi, lib = _lib()
    assert lib.igan_filter_image_bytes(*geom) == 0
    entries = _spaced(lib, 3)
    entries[2] = (W0, OUT0 + (1 << 24)) + geom + (0,)
    assert lib.igan_filter_images_grouped(None, _descs(_abi, entries), 3) == 1
    err = lib.igan_last_error()
    assert b'entry 2' in err and b'takes none' in err


def test_misaligned_out():
    _abi, lib = _lib()
    entries = _spaced(lib, 3)
    e = entries[1]
    entries[1] = (e[0], e[1] + 8) + e[2:]
    assert lib.igan_filter_images_grouped(None, _descs(_abi, entries), 3) == 1
    err = lib.igan_last_error()
    assert b'entry 1' in err and b'16-byte aligned' in err


def test_overlapping_out():
    _abi, lib = _lib()
    entries = _spaced(lib, 4)
    nbytes = int(lib.igan_filter_image_bytes(3, 3, 128, 128))
    entries[3] = (W0, entries[1][1] + (nbytes - 16)) + entries[3][2:]       # its first 16 bytes are entry 1's last
    assert lib.igan_filter_images_grouped(None, _descs(_abi, entries), 4) == 1
    err = lib.igan_last_error()
    assert b'entry 3' in err and b'overlaps entry 1' in err
    entries[3] = (W0, entries[1][1]) + entries[3][2:]                       # the same slice twice
    assert lib.igan_filter_images_grouped(None, _descs(_abi, entries), 4) == 1
    assert b'entry 3' in lib.igan_last_error()


def test_refusals_launch_nothing():
    _abi, lib = _lib()
    n = ctypes.c_ulonglong(7)
    assert lib.igan_debug_filter_image_launches(ctypes.byref(n), 1) == 0
    entries = _spaced(lib, 2)
    entries[1] = (W0, entries[0][1]) + entries[1][2:]
    assert lib.igan_filter_images_grouped(None, _descs(_abi, entries), 2) == 1
    assert lib.igan_debug_filter_image_launches(ctypes.byref(n), 0) == 0
    assert n.value == 0
    assert lib.igan_debug_filter_image_launches(None, 0) == 1
