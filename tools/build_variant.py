"""Build the HIP library as tools/var_NAME.so with the product's compile line
(native.build), for same-box A/B runs (tools/ab_chain.py, tools/with_lib.py):
    python tools/build_variant.py NAME [--rev REV] [-DMACRO[=V] ...]
--rev: the sources of that git revision (an archive of it in a temporary tree)
instead of this tree's: a kernel form since removed is built from a revision
that still has it, with the macro that selected it there."""
import argparse
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from diplomjourney_amd import native  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("name")
    ap.add_argument("--rev")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="MACRO[=V]")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tree:
        if a.rev:
            tar = subprocess.run(["git", "-C", REPO, "archive", a.rev, "diplomjourney_amd/csrc",
                                  "include"], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)
        print(native.build(True, a.defines, os.path.join(REPO, "tools", f"var_{a.name}.so"),
                           tree if a.rev else REPO))


if __name__ == "__main__":
    main()
