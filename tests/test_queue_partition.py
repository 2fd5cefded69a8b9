"""The path-queue partition kernels (csrc/queue_partition.hip: k_part_count, k_part_scan,
k_part_scatter) through pupil_debug_partition, against the exact stable-partition reference of
partition_cases.py.  Every comparison is array_equal on integers.

Each case first asserts the tile geometry the call reports (info: rounds, blocks, histogram
entries), so it cannot silently miss the regime it is named for, then that the scratch -- sized
for the capacity and filled with 0xA5A5A5A5, as the engine reuses it uncleared -- was written only
where it should be, then the outputs.  Regimes pinned: n = 0 (the memset path); partial waves,
blocks and tiles; the scan's second 16384-entry chunk and its carry (9 bins x 1821 blocks or
more); rounds 1, 2, 9 (a full batch of 8 key loads and a partial one) and 64; the rounds cap with
more blocks than the launch target; both clamps of PUPIL_PART_BLOCKS; bin masks; the running
64-bit totals with and without a snapshot.  The scan's third chunk needs 9 x 3641 blocks at 64
rounds, more than 59M paths: it is deliberately not covered here.

PUPIL_PART_BLOCKS is read once per process, so other launch targets run in fresh child
processes (python -m partition_cases), one after another; after a child that failed no further
one is started.

What the cases catch, by reading the kernel (neither mutation is committed):
  A. the scan's wave-scan guard `(int)__lane_id() >= o` turned into `> o`: lane o no longer adds
     lane 0's sum at any step, so every prefix of a wave lacks the 16 entries its lane 0 holds,
     and so do the wave totals and the chunk total.  A case fails when a selected path is counted
     in a histogram entry e (= bin * blocks + block) whose scan thread (e mod 16384) // 16 is a
     multiple of 64 -- entries 0..15 above all: bin 0 of the first 16 blocks, or, with one block,
     every bin.  That is every case with a non-empty list among uniform9, mod9, all0, runs,
     dropped, first_only and the flags patterns, from n = 1 up: `total` and the last bin's count
     (both come from the carry) are short, and with several blocks so are the starts and the ids
     of the later bins.  Cases whose lists are all empty (allFF, zero, n = 0, mask 1 << 9) pass,
     as they must.
  B. `carry += carry_s` dropped: the carry stays 0.  `total` and the last bin's count fail in
     every case with a non-empty list; the ids fail in the two-chunk cases, whose second chunk
     would restart at 0 -- 9 bins at n = 466177 (entry 16384 is the one past the first chunk),
     524288 and 4194305 (9 x 1821 = 16389 entries) -- in the bin whose histogram row reaches
     past entry 16384 (bin 8 in all three).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import partition_cases as P
from pupiloptixlab_amd import abi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = P.default_cases()


def check_record(case, info, failed, first):
    """info before everything else: the case ran in the regime it is named for"""
    assert tuple(info[:2]) == (case.rounds, case.blocks), \
        f"{case.name}: rounds, blocks = {tuple(info[:2])} (is PUPIL_PART_BLOCKS set in this process?)"
    assert info[2] == P.hist_entries(case.capacity) and case.nbins * info[1] <= info[2]
    assert info[3] == 1, f"{case.name}: scratch written outside the histogram or the id lists"
    assert not failed, f"{case.name}: {failed} differ from the reference, id list first at {first}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_partition_equals_the_reference(case):
    keys, cum = case.keys(), case.cum_in()
    rc, got = P.call(abi.load_library(), case.n, case.capacity, keys, case.nbins, case.mode, case.shift, case.mask,
                     cum, want_snap=case.totals == "snap")
    abi.check(rc)
    ref = P.reference(keys, case.nbins, case.mode, case.shift, case.mask, cum)
    failed, first = P.compare(got, ref)
    check_record(case, got["info"], failed, first)
    if case.n in (466177, 524288, 4194305) and case.nbins == 9:  # the scan ran its second chunk, with the carry
        assert P.SCAN_CHUNK < case.nbins * got["info"][1] <= 2 * P.SCAN_CHUNK
    # the variants of the totals were really exercised
    assert (got["cum_out"] is not None) == (case.totals != "none") and (got["snap"] is not None) == (case.totals == "snap")
    if case.n == 0:  # the memset path
        assert got["info"][1] == 0 and got["total"] == 0
        assert not got["counts"].any() and not got["starts"].any() and not got["log"].any()
        if cum is not None:
            assert np.array_equal(got["cum_out"], cum)
        if case.totals == "snap":
            assert np.array_equal(got["snap"], cum)


def test_named_regimes_are_in_the_table():
    """the sizes of the table by their literal figures (the cases assert them against info)"""
    g = {(c.n, c.nbins): (c.rounds, c.blocks, c.scan_chunks) for c in CASES if c.target == P.DEFAULT_TARGET}
    assert g[(466177, 9)] == (1, 1822, 2)   # 16398 entries: one past the scan's first chunk
    assert g[(524288, 9)] == (1, 2048, 2)
    assert g[(524289, 9)] == (2, 1025, 1)   # the last tile holds one path
    assert g[(4194305, 9)] == (9, 1821, 2)  # 16389 entries: two chunks again, at 9 rounds
    assert g[(1000, 9)] == (1, 4, 1) and g[(0, 9)] == (1, 0, 0)
    assert {c.n for c in CASES if c.capacity == 4194305 and c.n < c.capacity} == {0, 1, 1000, 524289}


def test_mask_zero_is_every_bin():
    keys = P.make_keys("uniform9", 1000, 11)
    lib = abi.load_library()
    rc0, a = P.call(lib, 1000, 1000, keys, 9, P.EXCLUSIVE, 0, 0)
    rc1, b = P.call(lib, 1000, 1000, keys, 9, P.EXCLUSIVE, 0, 0x1FF)
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["counts"], b["counts"]) and a["total"] == 1000


def test_optional_outputs_may_be_null():
    keys = P.make_keys("uniform9", 300, 12)
    lib = abi.load_library()
    out, counts, starts = np.zeros(300, np.uint32), np.zeros(9, np.uint32), np.zeros(9, np.uint32)
    p = lambda x: x.ctypes.data_as(abi.u32p)
    abi.check(lib.pupil_debug_partition(0, 300, 300, keys.ctypes.data_as(P.U8P), 9, 0, 0, 0, None, p(out), p(counts),
                                        p(starts), None, None, None, None, None))
    ref = P.reference(keys, 9, P.EXCLUSIVE, 0)
    assert np.array_equal(out, ref["out"]) and np.array_equal(counts, ref["counts"])
    assert np.array_equal(starts, ref["starts"])


# ------------------------------------------------------------------ other launch targets: child processes
_child_failed = []


@pytest.mark.parametrize("name", P.CHILD_LISTS)
def test_tile_geometry_under_part_blocks(name):
    assert not _child_failed, f"the child {_child_failed[0]} failed: no further one is started"
    value, cases = P.child_cases(name)
    _child_failed.append(name)  # cleared at the end: anything short of a clean pass stops the children
    env = os.environ.copy()
    env["PUPIL_PART_BLOCKS"] = value
    r = subprocess.run([sys.executable, "-m", "partition_cases", name], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=120)
    records = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    by_name = {rec["case"]: rec for rec in records}
    for case in cases:
        assert case.name in by_name, f"{case.name} did not run (exit {r.returncode}): {r.stderr[-2000:]}"
        rec = by_name[case.name]
        assert rec["error"] is None, rec
        check_record(case, rec["info"], rec["failed"], rec["first_mismatch"])
        assert rec["ok"]
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(records) == len(cases)
    if name == "blocks64":  # the regimes of this child, by their literal figures
        seen = {(c.n, by_name[c.name]["info"][0], by_name[c.name]["info"][1]) for c in cases}
        assert {(16384, 1, 64), (16385, 2, 33), (131073, 9, 57), (1048576, 64, 64), (1048577, 64, 65),
                (1064961, 64, 66)} <= seen
    elif name == "clamp_low":
        assert by_name[cases[0].name]["info"][:2] == [7, 56]      # the target of 64, not of 1
    else:
        assert by_name[cases[0].name]["info"][:2] == [2, 1172]    # the target of 2048, not of 99999
    _child_failed.clear()
