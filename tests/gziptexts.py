"""Seeded texts of the three kinds the text routes read, for the plain-gzip tests (CPU and GPU): FASTQ-like reads, a FASTA with
60-column lines, a GFA with long S lines.  No tests in here."""
import functools
import zlib

import numpy as np

KINDS = ("fastq", "fasta", "gfa")
LEVELS = (1, 6, 9)


def _bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _genome(rng, n):
    """bases with repeats in them (what makes an assembly compress): pieces of what came before come back, mutated"""
    out = bytearray(_bases(rng, min(n, 4000)))
    while len(out) < n:
        if rng.random() < 0.5:
            k = int(rng.integers(50, 3000))
            a = int(rng.integers(0, len(out) - 1))
            piece = bytearray(out[a:a + k])
            for i in rng.integers(0, max(len(piece), 1), len(piece) // 50):
                piece[int(i)] = b"ACGT"[int(rng.integers(0, 4))]
            out += piece
        else:
            out += _bases(rng, int(rng.integers(100, 3000)))
    return bytes(out[:n])


def fastq(rng, size):
    out, i = [], 0
    total = 0
    genome = _genome(rng, 200_000)
    while total < size:
        n = int(rng.integers(80, 260))
        a = int(rng.integers(0, len(genome) - n))
        qual = bytes(np.clip(rng.normal(36, 5, n), 2, 41).astype(np.uint8) + 33)
        rec = b"@read_%d/1 flowcell:%d\n" % (i, i % 7) + genome[a:a + n] + b"\n+\n" + qual + b"\n"
        out.append(rec); total += len(rec); i += 1
    return b"".join(out)[:size]


def fasta(rng, size):
    out, total, i = [], 0, 0
    while total < size:
        n = int(rng.integers(20_000, 200_000))
        seq = _genome(rng, n)
        rec = b">contig_%d len=%d\n" % (i, n) + b"\n".join(seq[k:k + 60] for k in range(0, n, 60)) + b"\n"
        out.append(rec); total += len(rec); i += 1
    return b"".join(out)[:size]


def gfa(rng, size):
    out, total, i = [b"H\tVN:Z:1.2\n"], 11, 0
    while total < size:
        n = int(rng.integers(5_000, 120_000))
        rec = b"S\tutig%d\t" % i + _genome(rng, n) + b"\tLN:i:%d\tRC:i:%d\n" % (n, n * 30)
        if i:
            rec += b"L\tutig%d\t+\tutig%d\t-\t0M\n" % (i - 1, i)
        out.append(rec); total += len(rec); i += 1
    return b"".join(out)[:size]


@functools.lru_cache(maxsize=None)
def text(kind, size):
    rng = np.random.default_rng({"fastq": 11, "fasta": 12, "gfa": 13}[kind] * 1_000_003 + size)
    return {"fastq": fastq, "fasta": fasta, "gfa": gfa}[kind](rng, size)


@functools.lru_cache(maxsize=None)
def raw_deflate(kind, size, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(text(kind, size)) + co.flush()


@functools.lru_cache(maxsize=None)
def gzip_file(kind, size, level):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    return co.compress(text(kind, size)) + co.flush()
