#!/usr/bin/env python3
"""record_tools_cli.py <tools-dir> <out.json>: the case table of tests/tools_cli_cases.py run against the executables of
<tools-dir>; exit code, stdout, stderr and the files written, per case.  tests/golden/tools_cli.json is this recording of
the build BEFORE the tool sources were split (tests/test_tools_cli.py replays it): it is not regenerated from later code."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import tools_cli_cases  # noqa: E402


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as work:
        got = tools_cli_cases.run_cases(os.path.abspath(sys.argv[1]), work)
    tools_cli_cases.dump(got, sys.argv[2])


if __name__ == "__main__":
    main()
