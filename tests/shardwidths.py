"""TEST INFRASTRUCTURE: one grid of window sizes at which the two multi-GPU wire formats are pinned — the shard message's
bit-packed window records (tiled_plan_core.h: shard_layout; field_bits = bit_width(w), 7 fields with -g / -e and 3 without,
window_bytes = ceil(fields x field_bits / 8)) and the full exchange's u16 wire (ts_batch_wire16_ok).

Every entry scans with `-c AAAAAA -x 0 -t 50`, so that a run of A matches at every position: a window of w A's holds
the nucleotide count w (all ones at w = 2^B - 1, the top bit alone at w = 2^(B-1)) and w - 5 canonical forward matches,
the largest values the fields can take.  tests/test_shard_results_cpu.py runs the grid through the host merge with
messages packed from oracle results, tests/test_gpu_shard_results.py through both device packers, and
tests/test_gpu_wire16.py holds the kernels' output against what ts_batch_wire16_ok promises."""
import ctypes as C
import functools

import numpy as np

from tests import seqgen

BASE = "-c AAAAAA -x 0 -t 50"
SCALE = 4                      # every match of a homopolymer is visible: the messages' variable sections at four times the plan's size

# (w, s, flags): every w > s entry keeps k <= min(s, w - s), which the planner requires
WIDTH_GRID = [
    (6, 6, "-r -g"), (7, 7, "-r -g"), (15, 15, "-r"), (16, 8, "-r -g"), (31, 31, "-r -g"), (32, 16, "-r"),
    (63, 21, "-r -g"), (64, 64, "-r -g"), (127, 127, "-r -e"), (128, 64, "-r"), (255, 85, "-r -g"),
    (256, 256, "-r -g"), (511, 511, "-r -g"), (512, 256, "-r -g"), (600, 300, "-r -g -e"), (1000, 500, "-r"),
    (1023, 341, "-r -g"), (1024, 512, "-r -g"), (2047, 2047, "-r -g"), (2048, 1024, "-r"), (4095, 1365, "-r -g"),
    (4096, 4096, "-r -g"), (8191, 8191, "-r -g"), (8192, 4096, "-r -g"), (10922, 5461, "-r -g"),
    (10923, 10923, "-r -g"), (16383, 5461, "-r -g"), (16384, 16384, "-r -g"), (32767, 32767, "-r -g"),
    (32768, 16384, "-r -g"), (32768, 32768, "-r"),
]


# At 11 and 12 bits x 7 fields the field that straddles bit 64 of a record is the NON-canonical count, which the grid's
# pattern set never raises (one pattern: every match is canonical).  The same inputs under `-c CCCCCC -p CCCCCC,AAAAAA`
# (the later -c holds): the run of A is a run of non-canonical matches, and that field holds w - 5.
NON_CANONICAL = "-c CCCCCC -p CCCCCC,AAAAAA"
SEAM_GRID = [(2047, 2047, "-r -g " + NON_CANONICAL), (2048, 1024, "-r -g " + NON_CANONICAL),
             (4095, 1365, "-r -g " + NON_CANONICAL)]


def entry_id(entry):
    w, s, flags = entry
    return "w%d-s%d%s" % (w, s, flags.replace(NON_CANONICAL, "-noncanonical").replace(" ", ""))


def cli(entry):
    w, s, flags = entry
    return "%s -w %d -s %d %s" % (BASE, w, s, flags)


def nuc_on(entry):
    return "-g" in entry[2].split() or "-e" in entry[2].split()


def field_bits(entry):
    return max(int(entry[0]).bit_length(), 1)


def window_bytes(entry):
    return ((7 if nuc_on(entry) else 3) * field_bits(entry) + 7) // 8


def inputs(opts):
    """(seqs, abs_pos): a run of A — three full windows with every field at its maximum and a short trailing one — and a
    chromosome long enough that a two-way split's boundary falls inside it, clear of both ends."""
    w = int(opts.window_size)
    homopolymer = b"A" * (3 * w + w // 2 + 5)
    chrom = seqgen.chromosome(np.random.default_rng(w), max(300_000, 12 * w + 17), opts.canonical_fwd, opts.canonical_rev, n_its=2)
    return [homopolymer, chrom], [0, 11]


@functools.lru_cache(maxsize=None)
def reference(command):
    """(opts, seqs, abs_pos, oracle results per segment) of `command`'s inputs: computed once, shared, never changed."""
    from teloscope_amd.cli import parse_cli
    from tests.backends import OracleBackend
    opts = parse_cli("x.fa " + command)
    seqs, abs_pos = inputs(opts)
    orac = OracleBackend(opts)
    return opts, seqs, abs_pos, [orac.scan_segment(s, abs_pos[i], opts.ultra_fast) for i, s in enumerate(seqs)]


def fill(plan, seqs, dev):
    """The plan's input buffer on the device, every segment at its offset."""
    import torch
    buf = torch.zeros(int(plan.info.input_bytes), dtype=torch.uint8, device=dev)
    for off, s in zip(plan.segment_offsets(), seqs):
        if len(s):
            buf[off:off + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8).to(dev)
    return buf


def scan_parts(plan, buf, dev):
    """Every part of the plan scanned on its own restricted batch (as a rank would): per part its (windows, stats,
    dense[:n]) as the export leaves them, and the record counts."""
    import torch
    from teloscope_amd.distributed import HipShard
    sptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    parts, counts = [], []
    for p in range(plan.world):
        r = plan.ranges[p]
        local = buf[r.input_begin:r.input_end].clone()         # a rank holds only the bytes its range reads
        hs = HipShard(plan, p, dev, slots=1)
        hs.scan(local.data_ptr(), sptr, 0)
        n = hs.finish(local.data_ptr(), sptr, 0)
        parts.append((hs.windows[0].clone(), hs.stats[0].clone(), hs.dense[0][:n].clone()))
        counts.append(n)
        hs.close()
    return parts, counts


# ---- what the grid covers, checked where it is defined
_bits = {field_bits(e) for e in WIDTH_GRID}
assert _bits == set(range(3, 17)), sorted(_bits)
assert {nuc_on(e) for e in WIDTH_GRID} == {True, False}
_bytes = {window_bytes(e) for e in WIDTH_GRID}
assert _bytes == set(range(2, 15)), sorted(_bytes)
assert any(field_bits(e) == 10 and nuc_on(e) for e in WIDTH_GRID) and any(field_bits(e) == 10 and not nuc_on(e) for e in WIDTH_GRID)
_ws = {e[0] for e in WIDTH_GRID}
_both = [B for B in range(3, 17) if (1 << B) - 1 in _ws and 1 << (B - 1) in _ws]       # all ones, and the top bit alone
assert len(_both) >= 6, _both
assert all(s == w or 6 <= min(s, w - s) for w, s, _ in WIDTH_GRID)
