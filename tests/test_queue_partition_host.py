"""The path-queue partition, host side (no GPU): the exact reference of partition_cases.py against
hand-written answers and against its own invariants, the case tables against the regimes they are
named for, and pupil_debug_partition's argument checks, which run before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import partition_cases as P
from pupiloptixlab_amd import abi

FF = 0xFF


# ------------------------------------------------------------------ the reference on hand-written keys
def test_exclusive_reference_by_hand():
    keys = [2, 0, FF, 2, 8, 9, 0, 2, 254, 1]
    r = P.reference(keys, 9, P.EXCLUSIVE, 0)
    assert [list(x) for x in r["ids"]] == [[1, 6], [9], [0, 3, 7], [], [], [], [], [], [4]]
    assert list(r["counts"]) == [2, 1, 3, 0, 0, 0, 0, 0, 1]
    assert list(r["starts"]) == [0, 2, 3, 6, 6, 6, 6, 6, 6]
    assert r["total"] == 7 and list(r["log"]) == list(r["counts"])
    assert list(r["out"]) == [1, 6, 9, 0, 3, 7, 4]  # 2, 5 and 8 (0xFF, 9, 254) are in no list


def test_exclusive_reference_with_shift_mask_and_fewer_bins():
    keys = [0x10, 0x1F, 0x00, 0x8F, 0x90, FF, 0x2A]
    r = P.reference(keys, 9, P.EXCLUSIVE, 4)
    assert [list(x) for x in r["ids"]] == [[2], [0, 1], [6], [], [], [], [], [], [3]]
    # a masked-out bin is empty even though keys name it; mask 0 is every bin; high bits do not exist
    keys = [0, 1, 2, 0, 1, 2, 3]
    assert list(P.reference(keys, 4, P.EXCLUSIVE, 0, mask=0b0101)["counts"]) == [2, 0, 2, 0]
    assert list(P.reference(keys, 4, P.EXCLUSIVE, 0, mask=0)["counts"]) == [2, 2, 2, 1]
    assert list(P.reference(keys, 4, P.EXCLUSIVE, 0, mask=0b110101)["counts"]) == [2, 0, 2, 0]
    assert list(P.reference(keys, 4, P.EXCLUSIVE, 0, mask=0b10000)["counts"]) == [0, 0, 0, 0]
    assert list(P.reference(keys, 3, P.EXCLUSIVE, 0)["out"]) == [0, 3, 1, 4, 2, 5]  # key 3 names no bin of three


def test_flags_reference_by_hand():
    tag = 5
    k = lambda bits, t=tag: (t << 2) | bits
    keys = [k(1), k(2), k(3), k(0), k(3, 4), 3, k(1)]
    r = P.reference(keys, 2, P.FLAGS, tag)
    assert [list(x) for x in r["ids"]] == [[0, 2, 6], [1, 2]]  # id 2 has both bits: it is in both lists
    assert list(r["starts"]) == [0, 3] and r["total"] == 5
    assert list(r["out"]) == [0, 2, 6, 1, 2]
    # tag 0: the key is its flag bits, and the key 0 is in no bin
    assert [list(x) for x in P.reference([0, 1, 2, 3, 0], 2, P.FLAGS, 0)["ids"]] == [[1, 3], [2, 3]]
    # tag 63 with both bits is the byte 0xFF, which only the exclusive mode treats as "none"
    assert P.reference([FF], 2, P.FLAGS, 63)["total"] == 2 and P.reference([FF], 9, P.EXCLUSIVE, 0)["total"] == 0


def test_totals_reference_is_uint64():
    cum = np.array([(1 << 40) - 1, (1 << 40) + 7], np.uint64)
    r = P.reference([(9 << 2) | 3] * 5, 2, P.FLAGS, 9, cum_in=cum)
    assert r["snap"].dtype == np.uint64 and list(r["snap"]) == [(1 << 40) - 1, (1 << 40) + 7]
    assert r["cum_out"].dtype == np.uint64 and list(r["cum_out"]) == [(1 << 40) + 4, (1 << 40) + 12]
    assert "snap" not in P.reference([0], 9, P.EXCLUSIVE, 0)


SMALL = [c for c in P.default_cases() if c.n <= 1000 and c.capacity <= 1000]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_reference_invariants(case):
    keys = case.keys()
    assert keys.dtype == np.uint8 and len(keys) == case.n
    r = P.reference(keys, case.nbins, case.mode, case.shift, case.mask, case.cum_in())
    k = keys.astype(np.uint32)
    live = P.live_bins(case.nbins, case.mask)
    for b, ids in enumerate(r["ids"]):
        assert np.all(np.diff(ids) > 0)  # increasing path order: the partition is stable
        assert b in live or len(ids) == 0
    if case.mode == P.EXCLUSIVE:  # the lists are disjoint and cover exactly the selected ids
        selected = np.flatnonzero((k != FF) & np.isin(k >> case.shift, live))
        assert np.array_equal(np.sort(r["out"]), selected)
    else:  # an id is in list b exactly when bit b is set under the matching tag: both bits, both lists
        both = np.flatnonzero(((k & 3) == 3) & ((k >> 2) == case.shift))
        assert np.all(np.isin(both, r["ids"][0])) and np.all(np.isin(both, r["ids"][1]))
        assert r["total"] == int((((k >> 2) == case.shift) * ((k & 1) + ((k >> 1) & 1))).sum())
    assert np.array_equal(r["starts"], np.concatenate([[0], np.cumsum(r["counts"])[:-1]]))
    # compare() accepts the reference's own answer laid out as the entry lays it out, and no other
    per = 2 if case.mode == P.FLAGS else 1
    out = np.full(per * case.n, P.FILL, np.uint32)
    out[:r["total"]] = r["out"]
    got = dict(r, out=out)
    assert P.compare(got, r) == ([], None)
    if r["total"] >= 2 and r["out"][0] != r["out"][1]:
        swapped = out.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        failed, first = P.compare(dict(r, out=swapped), r)
        assert "out" in failed and first == 0


def test_case_tables_reach_the_regimes_they_name():
    d = {c.name: c for c in P.default_cases()}
    assert len(d) == len(P.default_cases())  # names are unique
    by_n = lambda n: next(c for c in d.values() if c.n == n and c.nbins == 9)
    assert (by_n(466177).rounds, by_n(466177).blocks, 9 * by_n(466177).blocks) == (1, 1822, 16398)
    assert by_n(466177).scan_chunks == 2 and by_n(524288).scan_chunks == 2 and by_n(1000).scan_chunks == 1
    assert (by_n(524289).rounds, by_n(524289).blocks) == (2, 1025) and 524289 - 1024 * 512 == 1
    assert by_n(4194305).rounds == 9  # one full batch of 8 rounds and a partial one
    assert {c.rounds for c in d.values()} == {1, 2, 9}
    assert {c.totals for c in d.values()} == {"snap", "cum", "none"}
    assert P.hist_entries(4194305) == 18432
    env, cases = P.child_cases("blocks64")
    assert env == "64" and {c.rounds for c in cases} == {1, 2, 9, 64}
    assert any(c.rounds == 64 and c.blocks > 64 for c in cases)  # rounds capped: more blocks than the target
    assert 1064961 - 65 * 16384 == 1
    assert all(P.child_cases(n)[1] for n in P.CHILD_LISTS)


# ------------------------------------------------------------------ the entry point
def test_symbol_is_declared_and_exported():
    lib = abi.load_library()
    assert hasattr(lib, "pupil_debug_partition")
    assert "pupil_debug_partition" in abi.SIGNATURES
    assert lib.pupil_abi_version() == 7  # new entries are detected by symbol


def _args(**kw):
    a = dict(device=0, n=4, capacity=4, keys=np.zeros(4, np.uint8), nbins=9, mode=0, shift=0, mask=0, cum_in=None,
             out=np.zeros(8, np.uint32), counts=np.zeros(9, np.uint32), starts=np.zeros(9, np.uint32),
             total=np.zeros(1, np.uint32), log=np.zeros(9, np.uint32), cum_out=None, snap=None,
             info=np.zeros(4, np.uint32))
    a.update(kw)
    return a


def _call(a):
    p = lambda x, t: None if x is None else x.ctypes.data_as(C.POINTER(t))
    return abi.load_library().pupil_debug_partition(
        a["device"], a["n"], a["capacity"], p(a["keys"], C.c_uint8), a["nbins"], a["mode"], a["shift"], a["mask"],
        p(a["cum_in"], C.c_uint64), p(a["out"], C.c_uint32), p(a["counts"], C.c_uint32), p(a["starts"], C.c_uint32),
        p(a["total"], C.c_uint32), p(a["log"], C.c_uint32), p(a["cum_out"], C.c_uint64), p(a["snap"], C.c_uint64),
        p(a["info"], C.c_uint32))


U64 = np.zeros(9, np.uint64)
BAD_ARGUMENTS = {
    "null keys with n > 0": (dict(keys=None), b"null"),
    "null out": (dict(out=None), b"null"),
    "null counts": (dict(counts=None), b"null"),
    "null starts": (dict(starts=None), b"null"),
    "nbins 0": (dict(nbins=0), b"nbins"),
    "nbins 10": (dict(nbins=10), b"nbins"),
    "mode 2": (dict(mode=2), b"mode"),
    "flags mode with 9 bins": (dict(mode=1), b"two bins"),
    "flags mode with 1 bin": (dict(mode=1, nbins=1), b"two bins"),
    "n > capacity": (dict(n=4, capacity=3), b"capacity"),
    "capacity past 2^28": (dict(capacity=(1 << 28) + 1), b"capacity"),
    "snap without cum_in": (dict(snap=U64), b"cum_in"),
    "cum_out without cum_in": (dict(cum_out=U64), b"cum_in"),
}


@pytest.mark.parametrize("what", list(BAD_ARGUMENTS))
def test_argument_errors_are_codes_with_a_message(what):
    change, word = BAD_ARGUMENTS[what]
    a = _args(**change)
    before = {k: v.copy() for k, v in a.items() if isinstance(v, np.ndarray)}
    assert _call(a) == abi.ERR_INVALID
    assert word in abi.load_library().pupil_last_error()
    for k, v in before.items():  # refused before anything was written
        assert a[k] is None or np.array_equal(a[k], v), k
