"""CPU-side checks of the C-ABI: the library loads and exports every symbol
include/gnx_hip.h declares; without a HIP device creation fails loudly."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from geonomics_amd import _native, build
    if not os.path.exists(_native.LIB_PATH):
        build.build(verbose=False)
    return _native.load()


def declared_symbols():
    txt = open(os.path.join(ROOT, 'include', 'gnx_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(gnx_[a-z0-9_]+)\s*\(', txt)))


def test_every_declared_symbol_is_exported(lib):
    from geonomics_amd import _native
    syms = declared_symbols()
    assert len(syms) >= 35
    for s in syms:
        assert hasattr(lib, s), 'libgnxhip.so does not export %s' % s
    assert sorted(_native.EXPORTS) == syms


def test_struct_layouts_match_header(lib):
    from geonomics_amd import _native
    assert ctypes.sizeof(_native.Config) == 56
    sp = _native.default_species_params()
    assert ctypes.sizeof(sp) % 8 == 0
    assert lib.gnx_words_per_hom(1) == 16
    assert lib.gnx_words_per_hom(1024) == 16
    assert lib.gnx_words_per_hom(1025) == 32
    assert lib.gnx_words_per_hom(100000) == 1568


def test_no_cpu_fallback(lib):
    """Without a HIP device the product refuses to run (no silent fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('a HIP device is present')
    from geonomics_amd import _native
    with pytest.raises(_native.GnxError, match='no HIP device|hip'):
        _native.Device(8, 8, 1)


# ---- the signatures ctypes enforces are the header's (_native.parse_prototypes) ----

def test_every_prototype_is_declared_on_the_library(lib):
    from geonomics_amd import _native
    assert len(_native.PROTOTYPES) == 178 == len(declared_symbols())
    for name, (restype, argtypes) in _native.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert all(t is not None for t in argtypes), name


def test_argtypes_of_ten_prototypes_written_out_by_hand(lib):
    from geonomics_amd._native import Config
    P, i32, i64, f64, vp = ctypes.POINTER, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, \
        ctypes.c_void_p
    u64 = ctypes.c_uint64
    want = {
        'gnx_create': (ctypes.c_int, [P(Config), P(vp)]),
        'gnx_destroy': (None, [vp]),
        'gnx_last_error': (ctypes.c_char_p, []),
        'gnx_walk': (ctypes.c_int, [vp, i64, i32, i32]),
        'gnx_walk_history': (i64, [vp, i64, P(i64), P(i64), P(i64)]),
        'gnx_step_many': (ctypes.c_int, [P(vp), i32, i32, i32]),
        'gnx_cost_matrix': (ctypes.c_int, [vp, P(f64), f64, f64, i32, P(i32), P(f64)]),
        'gnx_tile2_route_ptrs': (ctypes.c_int, [vp, P(vp), P(vp), P(vp), P(vp)]),
        'gnx_admix_sweep': (ctypes.c_int, [vp, i64, P(i64), P(u64), i32, P(f64), P(f64), P(f64),
                                           P(f64), P(f64), P(f64), i32, i64]),
        'gnx_kin_pairs': (ctypes.c_int, [vp, i64, P(i64), P(u64), f64, i64, i64, i64, P(i64),
                                         P(i64), P(i64), P(i32), P(i32), P(i32), P(i32), P(i32)]),
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name


def test_a_type_outside_the_table_raises_and_names_the_prototype():
    from geonomics_amd import _native
    with pytest.raises(TypeError, match='gnx_x'):
        _native.parse_prototypes('int gnx_x(long double q);')
    with pytest.raises(TypeError, match='gnx_y'):
        _native.parse_prototypes('float gnx_y(int32_t a);')
    ok = _native.parse_prototypes('/* int gnx_no(void); */\nint gnx_z(const double* a /*[n]*/,\n'
                                  '          int64_t n);  // int gnx_no2(void);\n')
    assert ok == {'gnx_z': (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int64])}


def test_ctypes_refuses_a_wrong_argument_before_the_call(lib):
    """argument conversion comes first: nothing below reaches the library (the handle is null)"""
    import numpy as np
    from geonomics_amd._native import _ptr
    with pytest.raises(ctypes.ArgumentError):
        lib.gnx_words_per_hom(1.5)                       # a float for an int32_t
    slots32, out = np.zeros(1, np.int32), np.zeros((1, 2, 16), np.uint64)
    with pytest.raises(ctypes.ArgumentError):            # an int32 array for a const int64_t*
        lib.gnx_download_genomes(None, 1, _ptr(slots32), _ptr(out))
    with pytest.raises(ctypes.ArgumentError):            # a bare int for a typed pointer
        lib.gnx_download_genomes(None, 1, slots32.ctypes.data, _ptr(out))


def test_ptr_takes_its_type_from_the_array():
    import numpy as np
    from geonomics_amd._native import _ptr
    assert _ptr(None) is None
    for dt, ct in ((np.int32, ctypes.c_int32), (np.int64, ctypes.c_int64),
                   (np.uint64, ctypes.c_uint64), (np.uint8, ctypes.c_uint8),
                   (np.float32, ctypes.c_float), (np.float64, ctypes.c_double)):
        a = np.arange(3).astype(dt)
        p = _ptr(a)
        assert type(p) is ctypes.POINTER(ct)
        assert ctypes.addressof(p.contents) == a.ctypes.data and p[2] == 2
    with pytest.raises(KeyError):
        _ptr(np.zeros(3, np.int16))                      # no such pointer in the header
