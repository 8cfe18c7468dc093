"""What every loss-class call hands libsdeng.so -> ``launch_census.json``.

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.gen_launch_census                  (from the root of a checkout of commit 2bfc3b4, with this
                                                                                          script and tests/launch_census.py copied in: neither exists at that commit)
    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.gen_launch_census --full "eval dds_two_modes_d2"    prints the full records of the scenarios
                                                                                          whose label contains the text, as JSON, for diffing two trees

Recorded at commit 2bfc3b4, the last one where every loss class stated its step loop twice (``simulate()`` as launch parameters,
``__call__`` again as arguments of the gradient code) and ``engine.kl_adjoint`` / ``engine.cmcd_kl_adjoint`` compiled the control a second
time.  This is a record of how the fixture was made.  The recorder and the scenarios are ``tests/launch_census.py`` (public surface only, so
the same file runs at that commit and on later trees); no GPU is needed: the library is a stub.

The fixture holds, per scenario, one line per library call in call order: the entry point, the headline fields of its descriptor, and a
digest of the full record (every scalar argument, every scalar field of every structure recursively, which pointers are null, a SHA-256 of
the coefficient table behind ``coef``).
"""
from __future__ import annotations

import json
import os
import sys

from tests import golden_cases as gc
from tests import launch_census as lc

SOURCE = "commit 2bfc3b4"


def main(argv):
    if argv[:1] == ["--full"]:
        json.dump(lc.take(only=argv[1], full=True), sys.stdout, indent=1, sort_keys=True)
        return
    got = lc.take()
    with open(os.path.join(gc.GOLDEN_DIR, "launch_census.json"), "w") as f:
        json.dump(dict(source=SOURCE, scenarios=got), f, indent=0)
    print(len(got), "scenarios;", sum(len(v) for v in got.values()), "library calls")


if __name__ == "__main__":
    main(sys.argv[1:])
