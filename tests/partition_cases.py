"""The path-queue partition (csrc/queue_partition.hip) against an exact stable-partition reference:
the reference, the key patterns, the case tables and the call of pupil_debug_partition, shared by
test_queue_partition_host.py (CPU) and test_queue_partition.py (GPU).

The reference is the definition of the operation.  For each bin b below nbins whose mask bit is
set (mask 0: every bin; mask bits at or above nbins do not exist), ids_b = flatnonzero(in_bin(keys,
b)); a masked-out bin is empty even when keys name it.  Exclusive mode: in_bin = (k >> shift) == b
and k != 0xFF.  Flags mode: in_bin = ((k >> b) & 1) and (k >> 2) == tag.  counts = len(ids_b),
starts = their exclusive sum in bin order, total = their sum, log = counts, snap = cum_in, cum_out
= cum_in + counts (uint64), and out[starts[b] : starts[b] + counts[b]] = ids_b.  Everything is an
integer and every comparison is array_equal: there is no tolerance anywhere.

The tile geometry (rounds of 64 paths per wave, blocks of 4 waves) is restated here from the rule
the kernel file documents -- rounds = ceil(n / (256 * target)) clamped to 1..64, blocks = ceil(n /
(256 * rounds)), target = PUPIL_PART_BLOCKS clamped to 64..2048 -- so that each case can say
which regime it is in; the cases the tests name carry their figures as literals besides.

PUPIL_PART_BLOCKS is read once per process, so the cases under another launch target run in a
child:  python -m partition_cases LIST  (from this directory) runs the list of that name through
the debug entry and prints one JSON line per case -- {"case", "ok", "failed", "first_mismatch",
"info", "error"}; the exit status is 1 when a case failed.  Test infrastructure only.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child process starts without the suite's conftest
    sys.path.insert(0, ROOT)

EXCLUSIVE, FLAGS = 0, 1
MAX_BINS = 9
FILL = 0xA5A5A5A5          # what the debug entry fills its scratch with
DEFAULT_TARGET = 2048      # blocks a launch aims for; PUPIL_PART_BLOCKS is clamped to 64..2048
MAX_ROUNDS = 64
SCAN_CHUNK = 16384         # histogram entries the scan holds in LDS at a time
U8P, U64P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


# ------------------------------------------------------------------ the exact reference
def live_bins(nbins, mask):
    """the bins a key can land in"""
    every = (1 << nbins) - 1
    m = (mask & every) if mask else every
    return [b for b in range(nbins) if (m >> b) & 1]


def reference(keys, nbins, mode, shift_or_tag, mask=0, cum_in=None):
    k = np.asarray(keys, np.uint8).astype(np.uint32)
    ids = [np.zeros(0, np.int64) for _ in range(nbins)]
    for b in live_bins(nbins, mask):
        if mode == EXCLUSIVE:
            sel = ((k >> shift_or_tag) == b) & (k != 0xFF)
        else:
            sel = (((k >> b) & 1) != 0) & ((k >> 2) == shift_or_tag)
        ids[b] = np.flatnonzero(sel)
    counts = np.array([len(x) for x in ids], np.uint32)
    starts = (np.cumsum(counts, dtype=np.uint64) - counts).astype(np.uint32)
    ref = {"ids": ids, "counts": counts, "starts": starts, "total": int(counts.sum(dtype=np.uint64)),
           "log": counts.copy(), "out": np.concatenate(ids).astype(np.uint32)}
    if cum_in is not None:
        ref["snap"] = np.asarray(cum_in, np.uint64).copy()
        ref["cum_out"] = ref["snap"] + counts.astype(np.uint64)
    return ref


# ------------------------------------------------------------------ geometry and scratch size
def geometry(n, target=DEFAULT_TARGET):
    """(rounds, blocks) of a launch over n paths"""
    rounds = max(1, min(MAX_ROUNDS, -(-n // (256 * target))))
    return rounds, -(-n // (256 * rounds))


def hist_entries(capacity):
    return MAX_BINS * max(DEFAULT_TARGET, -(-capacity // (256 * MAX_ROUNDS)))


# ------------------------------------------------------------------ key patterns
def make_keys(pattern, n, seed, tag=0, tile=256):
    """n key bytes; tile = the paths of one block (256 * rounds), for the pattern that follows it"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    if pattern == "uniform9":           # every material bin
        k = rng.integers(0, 9, n)
    elif pattern in ("all0", "all8"):   # one bin holds every path
        k = np.full(n, int(pattern[3:]))
    elif pattern == "allFF":            # no path is in a bin
        k = np.full(n, 0xFF)
    elif pattern == "dropped":          # keys 9..254 name no bin: those paths are in no list
        k = np.where(rng.random(n) < 0.4, rng.integers(9, 255, n), rng.integers(0, 9, n))
    elif pattern == "last_only":        # one selected path, in the last tile's last live lane
        k = np.full(n, 0xFF)
        k[n - 1:] = 5
    elif pattern == "first_only":
        k = np.full(n, 0xFF)
        k[:1] = 3
    elif pattern == "runs":             # runs that fill a wave-round exactly, then a block tile exactly
        k = np.where(i < 2 * tile, (i // 64) % 9, (i // tile) % 9)
    elif pattern == "mod9":
        k = i % 9
    elif pattern == "bytes":            # any byte (exclusive mode with a shift; flags mode under tag 63)
        k = rng.integers(0, 256, n)
    elif pattern == "flags_random":     # the two flag bits at random under the matching tag
        k = (tag << 2) | rng.integers(0, 4, n)
    elif pattern == "flags_tags":       # three tags, one matches: stale flags of earlier bounces drop out
        k = (rng.choice([tag, (tag + 1) & 63, tag ^ 32], n) << 2) | rng.integers(0, 4, n)
    elif pattern == "flags_both":       # every path in both lists
        k = np.full(n, (tag << 2) | 3)
    elif pattern == "zero":
        k = np.zeros(n, np.int64)
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(k, dtype=np.uint8)


# ------------------------------------------------------------------ cases
class Case:
    """One call of the debug entry.  totals: "snap" (cum_in near 2^40, cum_out and snap asked
    for), "cum" (cum_in and cum_out, no snap: the partition gets no snapshot pointer) or "none".
    target: the launch target the case is meant to run under; rounds, blocks: what info must say."""

    def __init__(self, pattern, n, nbins=9, mode=EXCLUSIVE, shift=0, mask=0, totals="none", capacity=None,
                 target=DEFAULT_TARGET, geom=None, tag=""):
        self.pattern, self.n, self.nbins, self.mode, self.shift, self.mask = pattern, n, nbins, mode, shift, mask
        self.totals, self.capacity, self.target = totals, n if capacity is None else capacity, target
        self.rounds, self.blocks = geometry(n, target)
        if geom is not None:  # a figure the test names: the restatement above must agree with it
            assert geom == (self.rounds, self.blocks), (n, target, geom, (self.rounds, self.blocks))
        kind = "x" if mode == EXCLUSIVE else "f"
        self.name = "-".join(str(p) for p in (pattern, n, f"{kind}{nbins}", f"s{shift}", f"m{mask:x}", totals,
                                              f"cap{self.capacity}") if p != "") + (f"-{tag}" if tag else "")
        self.seed = sum(ord(c) * (j + 1) for j, c in enumerate(self.name))

    def keys(self):
        return make_keys(self.pattern, self.n, self.seed, self.shift if self.mode == FLAGS else 0, 256 * self.rounds)

    def cum_in(self):
        if self.totals == "none":
            return None
        rng = np.random.default_rng(self.seed + 1)
        return ((1 << 40) - rng.integers(0, 4 * max(self.n, 1), self.nbins)).astype(np.uint64)

    @property
    def scan_chunks(self):
        return -(-(self.nbins * self.blocks) // SCAN_CHUNK)


def _flags(pattern, n, tag, **kw):
    return Case(pattern, n, nbins=2, mode=FLAGS, shift=tag, **kw)


def default_cases():
    """the cases at the default launch target, in the test process"""
    c = []
    # sizes: every one with uniform keys; the totals variants take turns
    sized = [(0, (1, 0)), (1, (1, 1)), (63, (1, 1)), (64, (1, 1)), (65, (1, 1)), (255, (1, 1)), (256, (1, 1)),
             (257, (1, 2)), (1000, (1, 4)), (466177, (1, 1822)), (524288, (1, 2048)), (524289, (2, 1025)),
             (4194305, (9, 1821))]
    for j, (n, g) in enumerate(sized):
        c.append(Case("uniform9", n, totals=("snap", "cum", "none")[j % 3], geom=g))
    # the three totals variants at one small, one two-chunk size, and on the memset path
    for n in (0, 1000, 524288):
        for t in ("snap", "cum", "none"):
            c.append(Case("mod9", n, totals=t))
    # exclusive patterns, shift 0
    c += [Case("all0", 65), Case("all0", 524289, totals="snap"), Case("all8", 257), Case("all8", 466177),
          Case("allFF", 1), Case("allFF", 1000, totals="snap"), Case("allFF", 524288),
          Case("dropped", 255), Case("dropped", 1000), Case("dropped", 4194305),
          Case("last_only", 1), Case("last_only", 64), Case("last_only", 65), Case("last_only", 257),
          Case("last_only", 524289), Case("last_only", 4194305),
          Case("first_only", 1), Case("first_only", 1000), Case("first_only", 524289),
          Case("runs", 1000), Case("runs", 524288), Case("runs", 524289), Case("runs", 4194305, totals="snap"),
          Case("mod9", 63), Case("mod9", 256), Case("mod9", 466177), Case("mod9", 4194305)]
    # exclusive mode with a shift: the high nibble is the bin, 9..15 name none
    c += [Case("bytes", 257, shift=4), Case("bytes", 1000, shift=4), Case("bytes", 524289, shift=4, totals="snap")]
    # bin masks (0 = every bin is the rest of this table); a bit at or above nbins does not exist
    for n in (1000, 524289):
        for m in (0b1, 0b100000001, 0b010101010, 0b111111111, 0b1000000101, 0xFFFFFE00 | 0b10):
            c.append(Case("uniform9", n, mask=m, totals="cum"))
    c.append(Case("uniform9", 1000, mask=1 << 9))           # no bin below nbins is set: every list is empty
    # fewer bins than the keys name: keys at or above nbins are dropped
    c += [Case("uniform9", 1000, nbins=4), Case("uniform9", 524289, nbins=4, mask=0b110101, totals="snap"),
          Case("uniform9", 257, nbins=1), Case("mod9", 466177, nbins=5)]
    # flags mode
    c += [_flags("flags_random", n, 7, totals=t) for n, t in ((1, "none"), (64, "cum"), (65, "snap"), (1000, "none"),
                                                               (524289, "snap"), (4194305, "cum"))]
    c += [_flags("bytes", 1000, 63), _flags("bytes", 524288, 63),  # tag 63 with both bits is the byte 0xFF
          _flags("flags_tags", 257, 21), _flags("flags_tags", 524288, 21, totals="snap"),
          _flags("flags_tags", 4194305, 40),
          _flags("flags_both", 65, 9), _flags("flags_both", 256, 9), _flags("flags_both", 524289, 9, totals="snap"),
          _flags("zero", 257, 5), _flags("zero", 257, 0),
          # tag 0 and flag bits only: the filler key 0 of the lanes past n is in no bin
          _flags("flags_random", 65, 0), _flags("flags_random", 257, 0), _flags("flags_both", 65, 0),
          _flags("flags_both", 257, 0)]
    # scratch sized for a larger capacity, pre-filled, serves every smaller batch
    for n in (0, 1, 1000, 524289):
        c.append(Case("uniform9", n, capacity=4194305, totals="snap"))
        c.append(_flags("flags_random", n, 3, capacity=4194305, totals="snap"))
    return c


def child_cases(name):
    """the cases of one child process, and the PUPIL_PART_BLOCKS it runs under"""
    if name == "blocks64":
        t = 64
        table = [(16384, (1, 64)), (16385, (2, 33)), (131073, (9, 57)), (1048576, (64, 64)), (1048577, (64, 65)),
                 (1064961, (64, 66))]
        c = [Case("uniform9", n, totals="snap", target=t, geom=g) for n, g in table]
        c += [Case("runs", 131073, target=t, geom=(9, 57)), Case("runs", 1048577, target=t, geom=(64, 65)),
              Case("last_only", 1064961, target=t, geom=(64, 66)),
              _flags("flags_random", 16385, 11, target=t, geom=(2, 33)),
              _flags("flags_both", 1048577, 11, totals="snap", target=t, geom=(64, 65)),
              _flags("flags_tags", 1064961, 11, target=t, geom=(64, 66))]
        return "64", c
    if name == "clamp_low":   # 1 clamps to 64: unclamped, 100000 paths would take (64, 7)
        return "1", [Case("uniform9", 100000, totals="snap", target=64, geom=(7, 56))]
    if name == "clamp_high":  # 99999 clamps to 2048: unclamped, 600000 paths would take (1, 2344)
        return "99999", [Case("uniform9", 600000, totals="snap", target=2048, geom=(2, 1172))]
    raise KeyError(name)


CHILD_LISTS = ("blocks64", "clamp_low", "clamp_high")


# ------------------------------------------------------------------ the call and the comparison
def call(lib, n, capacity, keys, nbins, mode, shift_or_tag, mask=0, cum_in=None, want_cum=True, want_snap=True,
         want_info=True, device=0):
    """pupil_debug_partition; returns (return code, dict of what came back)"""
    per = 2 if mode == FLAGS else 1
    got = {"out": np.zeros(max(1, per * n), np.uint32), "counts": np.zeros(nbins, np.uint32),
           "starts": np.zeros(nbins, np.uint32), "total": np.zeros(1, np.uint32), "log": np.zeros(nbins, np.uint32),
           "info": np.zeros(4, np.uint32) if want_info else None,
           "cum_out": np.zeros(nbins, np.uint64) if cum_in is not None and want_cum else None,
           "snap": np.zeros(nbins, np.uint64) if cum_in is not None and want_snap else None}
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    u64 = lambda a: None if a is None else a.ctypes.data_as(U64P)
    cin = None if cum_in is None else np.ascontiguousarray(cum_in, np.uint64)
    kp = None if n == 0 else np.ascontiguousarray(keys, np.uint8).ctypes.data_as(U8P)
    rc = lib.pupil_debug_partition(device, n, capacity, kp, nbins, mode, shift_or_tag, mask, u64(cin), u32(got["out"]),
                                   u32(got["counts"]), u32(got["starts"]), u32(got["total"]), u32(got["log"]),
                                   u64(got["cum_out"]), u64(got["snap"]), u32(got["info"]))
    got["out"] = got["out"][:per * n]
    got["total"] = int(got["total"][0])
    return rc, got


def compare(got, ref):
    """(names of the outputs that differ from the reference, first index at which the id list does)"""
    failed = []
    for f in ("counts", "starts", "log", "snap", "cum_out"):
        if got.get(f) is not None and not (f in ref and np.array_equal(got[f], ref[f])):
            failed.append(f)
    if got["total"] != ref["total"]:
        failed.append("total")
    out, first = got["out"], None
    for b, ids in enumerate(ref["ids"]):  # each bin's list where the call says it is
        s, n = int(got["starts"][b]), int(got["counts"][b])
        if not np.array_equal(out[s:s + n], ids):
            failed.append(f"ids[{b}]")
    t = ref["total"]
    if not np.array_equal(out[:t], ref["out"]):  # the same, as one list
        failed.append("out")
        m = min(len(out), t)
        diff = np.flatnonzero(out[:m] != ref["out"][:m])
        first = int(diff[0]) if len(diff) else m
    if not np.array_equal(out[t:], np.full(max(0, len(out) - t), FILL, np.uint32)):  # nothing past the lists
        failed.append("tail")
    return failed, first


def run_case(lib, case):
    """one case through the debug entry -> the record the child prints"""
    keys, cum = case.keys(), case.cum_in()
    rc, got = call(lib, case.n, case.capacity, keys, case.nbins, case.mode, case.shift, case.mask, cum,
                   want_snap=case.totals == "snap")
    rec = {"case": case.name, "ok": False, "failed": [], "first_mismatch": None, "info": None, "error": None}
    if rc != 0:
        msg = lib.pupil_last_error()
        rec["error"] = f"{rc}: {msg.decode() if msg else ''}"
        return rec
    rec["info"] = [int(x) for x in got["info"]]
    rec["failed"], rec["first_mismatch"] = compare(got, reference(keys, case.nbins, case.mode, case.shift, case.mask, cum))
    rec["ok"] = not rec["failed"]
    return rec


def main(argv):
    from pupiloptixlab_amd import abi

    lib = abi.load_library()
    bad = 0
    for name in argv:
        for case in child_cases(name)[1]:
            rec = run_case(lib, case)
            print(json.dumps(rec), flush=True)
            if rec["error"]:  # a failed call may have left the device in error: nothing more is started
                return 1
            bad += not rec["ok"]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
