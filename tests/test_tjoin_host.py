"""The slot code of the per-group table join (dentist_amd/csrc/dh_tjoin.h: home slot, insert, probe walk, the -t cap
rule) compiled for the CPU (tests/native/tjoin_host.cpp) against a plain scan of the entry list: random keys with copies,
keys that share a home slot, at load factors up to the capacity the table is planned for.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def defines():
    hdr = open(os.path.join(ROOT, "dentist_amd", "csrc", "dh_tjoin.h")).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"#define (TJ_\w+) ([^/\n]+)", hdr)}


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libtjoin_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libtjoin_host.so"))
    L.tjoin_host_check.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_uint64]
    L.tjoin_host_check.restype = ctypes.c_int64
    return L


def test_the_table_is_planned_half_full_at_most():
    d = defines()
    assert int(d["TJ_CAP"]) == 8192 and int(d["TJ_SLOT_BITS"]) == 14  # 8 192 entries in 16 384 slots of 8 bytes = 128 KB


@pytest.mark.parametrize("n", [0, 1, 100, 2500, 8191, 8192])
@pytest.mark.parametrize("ndistinct", [1, 7, 300, 8192])
def test_lookups_equal_a_scan_of_the_entry_list(host, n, ndistinct):
    for tcap, strands in ((4, 3), (1, 1), (100000, 2), (0, 3)):
        assert host.tjoin_host_check(n, ndistinct, 28, 0, tcap, strands, 1000 * n + ndistinct) == 0


@pytest.mark.parametrize("n", [50, 2500, 8192])
def test_keys_of_one_home_slot(host, n):
    """every key hashes to the same home slot: one probe run that holds all entries"""
    assert host.tjoin_host_check(n, 5, 32, 1, 4, 3, n) == 0


def test_refuses_more_entries_than_planned(host):
    assert host.tjoin_host_check(8193, 5, 28, 0, 4, 3, 1) == -1
