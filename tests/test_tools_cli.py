"""The command-line surface of tools/ replayed against tests/golden/tools_cli.json: exit code, stdout, stderr and every file
written, byte for byte, for each case of tests/tools_cli_cases.py.  The golden file was recorded (scripts/record_tools_cli.py)
from the build before the tool sources were split over shared helpers; it is never regenerated from later code.  CPU only:
every case ends before a tool asks for a device."""
import os
import re

import pytest

import tools_cli_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tools_cli.json")


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    return tools_cli_cases.load(GOLDEN), tools_cli_cases.run_cases(TOOLS, str(tmp_path_factory.mktemp("cli")))


def test_the_table_is_the_recorded_one(replay):
    """(load has compared the digest of the case names)"""
    want, got = replay
    assert [g["case"] for g in got] == [w["case"] for w in want] and len(want) == len(tools_cli_cases.cases())


@pytest.mark.parametrize("field", ["exit", "stderr", "stdout", "files"])
def test_every_case_as_recorded(replay, field):
    want, got = replay
    diff = [(w["case"], w[field], g[field]) for w, g in zip(want, got) if w[field] != g[field]]
    assert not diff, "%d cases differ, the first: %r\nrecorded: %r\nnow:      %r" % ((len(diff),) + diff[0])


def test_no_case_asks_for_a_device(replay):
    """(on a machine without a GPU a case that reached dh_ctx_create would say so)"""
    want, got = replay
    for r in want + got:
        assert not re.search(r"HIP|hip|device|dh_ctx_create", r["stderr"]), r["case"]


def test_every_outcome_is_seen(replay):
    """the table is worth its name only while it reaches the usage exits, the library's failures and successes that write"""
    want, _ = replay
    assert {r["exit"] for r in want} >= {0, 1, 2}
    assert sum(bool(r["files"]) for r in want) >= 20
    assert sum(r["stderr"].count("have no effect here") == 1 for r in want) >= 60
    assert not any(r["stderr"].count("have no effect here") > 1 for r in want)


def test_the_unknown_tool_message_names_the_makefiles_tools(replay):
    """the table of main() and DAZZ_TOOLS of the Makefile are the two lists of tool names: they agree, in order"""
    _, got = replay
    with open(os.path.join(ROOT, "Makefile")) as f:
        names = re.search(r"^DAZZ_TOOLS := (.*)$", f.read(), re.M).group(1).split()
    msg = next(r["stderr"] for r in got if r["case"].startswith("2: dazz_tools --tool nope"))
    assert re.fullmatch(r"nope: unknown tool \(expected (.*)\)\n", msg).group(1).split() == names
    assert len(names) == len(set(names)) == 29
