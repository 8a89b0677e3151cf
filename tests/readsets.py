"""Pattern sets and reads shared by tests/test_gpu_read_batch_general.py and tests/test_gpu_read_routes_general.py: the sets of
the read filter that the tiled kernel does not take, the reads of test_read_filter_on_pattern_sets_outside_the_tiled_kernel
(tests/test_gpu_shards_fullsize.py) with edge lengths added, and the dense set that overflows the general kernels' tile slots.
The oracle's verdicts are computed once per set and shared."""
import functools

import numpy as np

from tests import harness as H

# the five sets of test_read_filter_on_pattern_sets_outside_the_tiled_kernel and a canonical 9-mer with its one-mismatch
# variants: the table form with two lengths, k = 9 and 10, the wide form with nine lengths, and a 42-base pattern
SETS = [
    "-p TTAGGG,TTAGG",
    "-c TTAGGGTTA -x 0 -l 30",
    "-c AACCCTAACC -x 1",
    "-x 0 -p TTAG,TTAGG,TTAGGG,TTTAGGG,TTTTAGGG,TTAGGGTTA,TTAGGGTTAG,TTAGGGTTAGG,TTAGGGTTAGGG",
    "-c TTAGGG -x 0 -p TTAGGG," + "TTAGGG" * 7,
    "-c TTTTTAGGG -x 1",
]
SET_IDS = ["mixed_5_6", "k9", "k10", "wide_nine_lengths", "wide_42_bases", "k9_x1"]

# lengths around the 16-byte step of the input layout, around one and two tiles of the general kernels (TS_GENERAL_TILE = 4096)
EDGE_LENGTHS = [1, 4, 5, 6, 15, 16, 17, 4095, 4096, 4097, 8192, 8193]

# a homopolymer under two pattern lengths puts two records on a position: more than a tile's slot holds at first
OVERFLOW_SET = "-c AAAAAA -p AAAAAA,AAAAA -x 0"

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def options(flags):
    return H.parse_cli("--fastq-subset " + flags)


def random_bases(rng, n):
    return bytes(rng.choice(_ACGT, size=int(n)))


def reads_for(flags):
    """60 reads of 200-4000 random bases, every third with 3-39 forward units in front, every third with reverse units
    behind (default_rng(7), as the test these come from); then every edge length twice: the canonical unit repeated and cut,
    and random bases."""
    opts = options(flags)
    rng = np.random.default_rng(7)
    unit_f, unit_r = opts.canonical_fwd.encode(), opts.canonical_rev.encode()
    reads = []
    for i in range(60):
        body = random_bases(rng, rng.integers(200, 4000))
        if i % 3 == 0:
            body = unit_f * int(rng.integers(3, 40)) + body
        elif i % 3 == 1:
            body = body + unit_r * int(rng.integers(3, 40))
        reads.append(body)
    for n in EDGE_LENGTHS:
        reads.append((unit_f * (n // len(unit_f) + 1))[:n])
        reads.append(random_bases(rng, n))
    return reads


@functools.lru_cache(maxsize=None)
def oracle_passes(flags):
    """OracleReadFilter's verdicts on reads_for(flags), computed once."""
    from tests.backends import OracleReadFilter
    return tuple(OracleReadFilter(options(flags)).filter(reads_for(flags)))


def overflow_reads():
    rng = np.random.default_rng(17)
    r = lambda n: random_bases(rng, n)      # noqa: E731
    return [b"A" * 9000, r(3000) + b"A" * 5000, r(6000), b"T" * 4097, r(100) + b"A" * 30 + r(100), b"A" * 41, b"A" * 42, b"A" * 43,
            r(5000) + b"T" * 4200 + r(5000)]


def fastq_records(reads, eol=b"\n"):
    return [b"@r%d" % i + eol + r + eol + b"+" + eol + b"I" * len(r) + eol for i, r in enumerate(reads)]


def fastq_text(reads, eol=b"\n"):
    return b"".join(fastq_records(reads, eol))
