"""k_tile's column loop on 32-bit words without a GPU: dentist_amd/csrc/dh_tile.h (tile_block / tile_col_h, the
three-input functions of dh_bitvec.h evaluated by their truth tables on the host) compiled for the CPU
(tests/native/bitvec_host.cpp) against the 64-bit reference step dh_tile.h: tile_col on random tiles.  Bit-exact in
Pv, Mv, wild, z, dbot and lv."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bv_lib():
    path = os.path.join(ROOT, "tests", "native", "libdh_bitvec_host.so")
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libdh_bitvec_host.so"], check=True)
    L = ctypes.CDLL(path)
    L.dh_bitvec_tile_check.restype = ctypes.c_long
    L.dh_bitvec_tile_check.argtypes = [ctypes.c_uint64, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.dh_bitvec_b3_check.restype = ctypes.c_long
    L.dh_bitvec_b3_check.argtypes = [ctypes.c_uint64, ctypes.c_long]
    return L


def test_b3_tables(bv_lib):
    assert bv_lib.dh_bitvec_b3_check(1, 100_000) == 0


@pytest.mark.parametrize("wb,tan", [(64, 0), (64, 1), (32, 0), (32, 1)])
def test_column_loop_equals_reference_step(bv_lib, wb, tan):
    stats = np.zeros(8, dtype=np.int64)
    bad = bv_lib.dh_bitvec_tile_check(11 + wb + tan, 24_000, wb, tan, stats.ctypes.data)
    assert bad == 0, f"{bad} of {stats[0]} tiles differ"
    tiles, cols, nowild, zcross, full, past32, idle = (int(x) for x in stats[:7])
    assert cols >= 1_000_000, cols
    # every path of the loop was taken, many times
    for name, v in (("no-wild", nowild), ("z crossing zero", zcross), ("full", full), ("past 32 columns", past32),
                    ("idle lanes", idle)):
        assert v >= 500, (name, v, tiles)
