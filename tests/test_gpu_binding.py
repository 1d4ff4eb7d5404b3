"""A 64-bit by-value argument survives the binding (geonomics_amd/_native.py declares every
prototype of include/gnx_hip.h to ctypes: an int64_t is passed whole, not as a C int)."""
import pytest

from geonomics_amd import _native as nat

pytestmark = pytest.mark.gpu


def test_int64_by_value_arguments_pass_whole():
    dev = nat.Device(8, 8, 1, cap_inds=1024)
    try:
        dev.step_index = 2 ** 40 + 3
        assert dev.step_index == 2 ** 40 + 3
        dev.set_max_id(2 ** 40)
    finally:
        dev.close()
