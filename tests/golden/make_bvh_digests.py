"""Records the builder's output for tests/test_bvh_build_identity.py (needs the GPU; run from the
repo root on the commit whose trees are to be pinned):

    python tests/golden/make_bvh_digests.py <commit hash> [output path]

Writes tests/golden/bvh4_digests.json: {"commit": ..., "cases": {case: digest}} with the cases and
the digest function of the test module itself.  Run it only when the builder's output is meant to
change; a restructuring of the builder is checked against the file as it stands.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_bvh_build_identity as ident  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else ident.DIGESTS
    cases = {}
    for case in ident.CASES:
        mp = pytest.MonkeyPatch()
        try:
            cases[case] = ident.digest(case, mp)
        finally:
            mp.undo()
        print(case, cases[case], flush=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(cases)} digests to {out}")


if __name__ == "__main__":
    main()
