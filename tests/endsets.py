"""Inputs and expectations shared by tests/test_gpu_terminal_ends_general.py: for every pattern set of tests/readsets.py the
context's options (-t 2000 -d 100 -l 30), the segments — the set's reads and thirteen shapes that place terminal blocks on
either side of walkSegment's rule (src/input.cpp:849-853) — and the CPU oracle's terminal blocks reduced per side, computed
once per set."""
import functools
import re

import numpy as np

from tests import harness as H
from tests import readsets as R

TAIL = " -t 2000 -d 100 -l 30"


def cli(flags):
    """The set's flags without its own -l, under the terminal limit, block distance and block length of these tests."""
    return "x " + re.sub(r"\s*-l \d+", "", flags) + TAIL


def options(flags):
    return H.parse_cli(cli(flags))


def shapes(fwd, rev):
    """Thirteen segments around the side rule.  fwd / rev: the unit that counts in the walk from the start / from the end.
    1-4: two blocks on one side, the longer one first and then second; 5, 12: both sides; 6: a block of the forward walk that
    lands on the end side; 7: a block of the reverse walk on the start side; 8: one block from each walk in a short segment; 9,
    10: either side of the tie (the tie goes to the start side); 11: the reverse unit in the middle; 13: nothing terminal."""
    rng = np.random.default_rng(41)
    r = lambda n: R.random_bases(rng, n)        # noqa: E731
    F, Rv = fwd, rev
    return [
        F * 60 + r(300) + F * 20 + r(5000),
        F * 20 + r(300) + F * 60 + r(5000),
        r(5000) + Rv * 20 + r(300) + Rv * 60,
        r(5000) + Rv * 60 + r(300) + Rv * 20,
        F * 40 + r(3000) + Rv * 25,
        r(700) + F * 50,
        Rv * 50 + r(700),
        F * 30 + r(40) + Rv * 30,
        r(100) + F * 50 + r(100),
        r(101) + F * 50 + r(100),
        r(100) + Rv * 50 + r(100),
        F * 40 + r(6000) + Rv * 25,
        r(2500) + F * 50 + r(2500),
    ]


N_SHAPES = 13


@functools.lru_cache(maxsize=None)
def segments(flags):
    """-> (segments, absolute positions): R.reads_for(flags), then the thirteen shapes; every third segment lies at a
    non-zero absolute position."""
    opts = options(flags)
    segs = list(R.reads_for(flags)) + shapes(opts.canonical_fwd.encode(), opts.canonical_rev.encode())
    abs_pos = [1_000_003 * (i + 1) if i % 3 == 0 else 0 for i in range(len(segs))]
    return tuple(segs), tuple(abs_pos)


def per_side(blocks, n, abs_pos):
    """The terminal blocks of a segment of n bases reduced as walkSegment reduces them (tests/test_gpu_terminal_ends.py)."""
    best = [0, 0]
    for b in blocks:
        rel, ln = int(b["start"]) - abs_pos, int(b["block_len"])
        side = 0 if rel <= n - (rel + ln) else 1
        best[side] = max(best[side], ln)
    return best


@functools.lru_cache(maxsize=None)
def oracle_ends(flags):
    """The CPU oracle's tips-only terminal blocks of segments(flags), reduced per side: an (n, 2) uint32 array, read-only."""
    from tests.backends import OracleBackend
    orac = OracleBackend(options(flags))
    segs, abs_pos = segments(flags)
    out = np.array([per_side(orac.scan_segment(s, a, True)["terminal_blocks"], len(s), a) for s, a in zip(segs, abs_pos)],
                   dtype=np.uint32).reshape(len(segs), 2)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_block_counts(flags):
    """Per segment, how many terminal blocks the oracle calls (the shapes with two blocks on one side need two)."""
    from tests.backends import OracleBackend
    orac = OracleBackend(options(flags))
    segs, abs_pos = segments(flags)
    return tuple(len(orac.scan_segment(s, a, True)["terminal_blocks"]) for s, a in zip(segs, abs_pos))


def assert_classes(flags):
    """The cases these inputs are there for occur — by the oracle's answer, not the product's."""
    exp = oracle_ends(flags)
    sh = exp[-N_SHAPES:]
    nb = oracle_block_counts(flags)[-N_SHAPES:]
    assert nb[0] == nb[1] == nb[2] == nb[3] == 2, nb                # two blocks on one side, the longer one first and second
    assert all(sh[i][0] >= 360 and sh[i][1] == 0 for i in (0, 1))   # (the longer of the two: 60 units)
    assert all(sh[i][1] >= 360 and sh[i][0] == 0 for i in (2, 3))
    assert all(sh[i][0] > 0 and sh[i][1] > 0 for i in (4, 11))      # both sides
    assert sh[5][0] == 0 and sh[5][1] > 0                           # a forward-walk block on the end side
    assert sh[6][0] > 0 and sh[6][1] == 0                           # a reverse-walk block on the start side
    assert sh[8][0] > 0 and sh[8][1] == 0                           # either side of the tie: the start side,
    assert sh[9][0] == 0 and sh[9][1] > 0                           # and one base further the end side
    assert list(sh[12]) == [0, 0]
    reads = exp[:-N_SHAPES]
    n_start, n_end = int((reads[:, 0] > 0).sum()), int((reads[:, 1] > 0).sum())
    n_empty = int(((reads[:, 0] == 0) & (reads[:, 1] == 0)).sum())
    print("%s: reads with a start side %d, with an end side %d, empty %d" % (flags, n_start, n_end, n_empty))
    assert n_start >= 20 and n_end >= 15 and n_empty >= 30, (n_start, n_end, n_empty)
