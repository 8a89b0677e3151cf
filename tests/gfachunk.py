"""What tests/test_gfa_chunk_reference_cpu.py, tests/test_gpu_gfa_chunk.py and tests/test_gpu_gfa_device.py share: a plain-Python
sequential restatement of the GFA framing rules (ref_walk) and of the host's graph build (ref_dump), seeded generators of GFA
text with their edge cases, and a thin ctypes wrapper over ts_gfa_chunk_walk, ts_chunk_data and ts_chunk_carry_over.  No test
functions live here.

The references restate readGfa (include/teloscope_mi355x_gfa.hpp), not the kernels: they go through the text line by line and
split every line at its tabs.  The device does the same with a line index, a tab index and prefix sums over lines."""
import ctypes as C
import random
import re

from tests import fastachunk as F

TAB, CR = 9, 13


# ------------------------------------------------------------------------------------------------------------ references
def ref_walk(text, at_end):
    """-> (segments, lines, text, next, foreign).  A segment is (off, len, n_fields, f1_at, f1_len, f2_at, f2_len, f3_at, f3_len,
    name_at, star) as ts_gfa_segment holds it, a line (off, len, kind, text_at) as ts_gfa_line does; text is the segments' names
    and the P / H lines one behind the other in input order; foreign is (off, first-field length) of the lowest foreign line
    or None."""
    text = bytes(text)
    n, p = len(text), 0
    segs, lines, gathered, foreign = [], [], bytearray(), None
    while p < n:
        nl = text.find(b"\n", p)
        if nl < 0 and not at_end:
            break                                               # an unfinished last line: the carry
        e, q = (n, n) if nl < 0 else (nl, nl + 1)
        if e > p and text[e - 1] == CR:
            e -= 1
        if e > p:
            c = text[p:e]
            t, single = c[:1], len(c) == 1 or c[1] == TAB
            if t != b"#" and not (single and t in (b"H", b"S")) and foreign is None:
                foreign = (p, len(c.split(b"\t", 1)[0]))
            if single and t == b"S":
                f = c.split(b"\t", 4)
                if len(f) >= 3:
                    at = [0]
                    for x in f[:-1]:
                        at.append(at[-1] + len(x) + 1)
                    f3 = (at[3], len(f[3])) if len(f) >= 4 else (0, 0)
                    star = (1 if f[2] == b"*" else 0) | (2 if len(f) >= 4 and f[3] == b"*" else 0)
                    segs.append((p, len(c), len(f), at[1], len(f[1]), at[2], len(f[2]), f3[0], f3[1], len(gathered), star))
                    gathered += f[1]
            elif single and t in (b"P", b"H"):
                lines.append((p, len(c), t[0], len(gathered)))
                gathered += c
        p = q
    return segs, lines, bytes(gathered), (n if at_end else p), foreign


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for c in data:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def ref_graph(text, path):
    """The host's graph build from ref_walk's tables: -> dict(version, has_version, segments [(name, sequence or None)], paths
    [(name, [(component, orientation)])], edits [(off, len, text)]) or dict(error=message)."""
    text = bytes(text)
    segs, lines, gathered, nxt, foreign = ref_walk(text, True)
    assert nxt == len(text)
    version, has_version, headers, paths = 1, False, [], []
    for off, ln, kind, at in lines:
        c = gathered[at:at + ln]
        assert c == text[off:off + ln]
        f = c.split(b"\t")
        if kind == ord("H"):
            for x in f[1:]:
                if x.startswith(b"VN:Z:"):
                    has_version, version = True, 2 if x[5:6] == b"2" else 1
                    headers.append((off, ln))
        else:
            f = c.split(b"\t", 3)
            if len(f) >= 3:
                comps = [(x[:-1], x[-1:]) for x in re.split(b"[,;]", f[2]) if len(x) >= 2]
                paths.append((f[1], comps))
    if version == 2 and foreign is not None:
        return dict(error=b"GFA 2 record type '%s' in '%s' is not supported: only H and S records of a GFA 2 graph are read." % (
            text[foreign[0]:foreign[0] + foreign[1]], str(path).encode()))
    edits = [(off, ln, b"H\tVN:Z:1.2") for off, ln in headers if b"VN:Z:2" in text[off:off + ln]]
    out, seen = [], set()
    for off, ln, nf, a1, l1, a2, l2, a3, l3, name_at, star in segs:
        name = gathered[name_at:name_at + l1]
        assert name == text[off + a1:off + a1 + l1]
        so, sl = a2, l2
        if version == 2 and nf >= 4:
            so, sl = a3, l3
            edits.append((off + a2, a3 - a2, b""))
        seq = text[off + so:off + so + sl]
        assert (seq == b"*") == bool(star & (2 if (version == 2 and nf >= 4) else 1))
        if name in seen:
            return dict(error=b"segment '%s' is defined twice in '%s'." % (name, str(path).encode()))
        seen.add(name)
        out.append((name, None if seq == b"*" else seq))
    return dict(version=version, has_version=has_version, segments=out, paths=paths, edits=sorted(edits))


def ref_dump(text, path):
    """ref_graph in the form tests/cpp/gfa_device_cli.cpp --dump-records prints."""
    g = ref_graph(text, path)
    if "error" in g:
        return b"error\t" + g["error"] + b"\n"
    out = [b"version\t%d\t%d\n" % (g["version"], 1 if g["has_version"] else 0)]
    for name, seq in g["segments"]:
        out.append(b"S\t%s\t%s\t%016x\n" % (name, b"*" if seq is None else b"%d" % len(seq), fnv1a64(seq or b"")))
    for name, comps in g["paths"]:
        out.append(b"P\t" + name + b"".join(b"\t" + c + b"\t" + o for c, o in comps) + b"\n")
    for off, ln, txt in g["edits"]:
        out.append(b"E\t%d\t%d\t%s\n" % (off, ln, txt))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------------------ generators
def bases(gen, n, cap=None):
    """n random bases; cap 'start' / 'end' / 'both' puts telomere repeats on that side (when there is room)."""
    out = bytearray(gen.choice(b"ACGT") for _ in range(n))
    k = min(n // 3, 300) // 6 * 6
    if cap in ("start", "both") and k:
        out[:k] = b"CCCTAA" * (k // 6)
    if cap in ("end", "both") and k:
        out[n - k:] = b"TTAGGG" * (k // 6)
    return bytes(out)


def pathless_graph(seed, n_segments=3000, lo=50, hi=2000):
    """S lines only (with a few tags), a tenth of them telomere-capped."""
    gen = random.Random(seed)
    out = [b"H\tVN:Z:1.0\n"]
    for i in range(n_segments):
        cap = ("start", "end", "both")[i % 3] if i % 10 == 3 else None
        seq = bases(gen, gen.randrange(lo, hi), cap)
        out.append(b"S\tutg%06dl\t%s%s\n" % (i, seq, b"\tLN:i:%d\trd:i:%d" % (len(seq), i % 7) if i % 4 else b""))
    return b"".join(out)


def path_graph(seed, n_segments=1200, n_paths=40, lo=200, hi=3000):
    """P lines first, then S and L lines, the H line last."""
    gen = random.Random(seed)
    names = [b"s%d" % i for i in range(n_segments)]
    out = []
    per = n_segments // n_paths
    for k in range(n_paths):
        comps = [names[k * per + j] + (b"+" if gen.random() < 0.6 else b"-") for j in range(per)]
        out.append(b"P\tpath%d\t%s\t*\n" % (k, (b";" if k % 5 == 0 else b",").join(comps)))
    for i, nm in enumerate(names):
        first, last = i % per == 0, i % per == per - 1
        cap = "both" if first or last else "start" if i % 7 == 3 else None      # (a path end counts on either side, by orientation)
        out.append(b"S\t%s\t%s\n" % (nm, bases(gen, gen.randrange(lo, hi), cap)))
        if i:
            out.append(b"L\t%s\t+\t%s\t+\t0M\n" % (names[i - 1], nm))
    out.append(b"H\tVN:Z:1.1\n")
    return b"".join(out)


def mixed_lines(seed, n, kinds=b"SPHL#e"):
    """n short lines of the given kinds (e: empty), every kind's count crossing the slices of 2 048 lines."""
    gen = random.Random(seed)
    out = []
    for i in range(n):
        k = kinds[gen.randrange(len(kinds))]
        if k == ord("S"):
            out.append(b"S\tn%d\t%s%s\n" % (i, b"ACGT"[:1 + i % 4], b"\tx" * (i % 4)))
        elif k == ord("P"):
            out.append(b"P\tp%d\tn%d+,n%d-\t*\n" % (i, i, i + 1))
        elif k == ord("H"):
            out.append(b"H\tc%d:Z:x\n" % i)
        elif k == ord("L"):
            out.append(b"L\ta\t+\tb\t-\t0M\n")
        elif k == ord("#"):
            out.append(b"# %d\n" % i)
        else:
            out.append(b"\r\n" if i % 2 else b"\n")
    return b"".join(out)


def edge_cases():
    """name -> complete text."""
    gen = random.Random(7)
    a, b, c = bases(gen, 400, "start"), bases(gen, 333, "end"), bases(gen, 90)
    three = b"S\ta\t%s\nS\tb\t%s\nS\tc\t%s\n" % (a, b, c)
    cases = {}
    cases["empty"] = b""
    cases["only blank lines"] = b"\n\r\n\n"
    cases["comment lines"] = b"# a comment\n#\tS\tx\tACGT\n" + three + b"#"
    cases["last line without newline"] = b"H\tVN:Z:1.0\nS\ta\t%s\nS\tb\t%s" % (a, b)
    cases["last line ending in cr without newline"] = b"S\ta\t%s\nS\tb\t%s\r" % (a, b)
    cases["S alone"] = b"S\n" + three + b"S"
    cases["S and a tab"] = b"S\t\n" + three
    cases["S with two fields"] = b"S\tx\n" + three + b"S\ty\r\n"
    cases["S with a star"] = b"S\ta\t*\nS\tb\t%s\nS\tc\t*\tLN:i:5\n" % b
    cases["S with an empty sequence"] = b"S\ta\t\nS\tb\t%s\nS\tc\t\tLN:i:0\n" % b
    cases["empty name"] = b"S\t\t%s\nS\tb\t%s\n" % (a, b)
    cases["SX is not single"] = b"SX\ta\t%s\n" % a + three
    cases["S with nine tabs"] = b"S\ta\t%s\tLN:i:400\tRC:i:1\tx\ty\tz\tw\tv\nS\tb\t%s\t\t\t\t\n" % (a, b)
    cases["gfa2 with and without tags"] = b"H\tVN:Z:2.0\nS\ta\t400\t%s\tRC:i:5\txx:Z:y\nS\tb\t333\t%s\n" % (a, b)
    cases["gfa2 with three fields only"] = b"H\tVN:Z:2.0\nS\ta\t%s\nS\tb\t*\nS\tc\t90\t%s\n" % (a, c)
    cases["gfa2 stars"] = b"H\tVN:Z:2.0\nS\ta\t8\t*\nS\tb\t1\t*\tx\nS\tc\t*\t%s\nS\td\t*\n" % c
    cases["gfa2 header as the last line"] = b"S\ta\t400\t%s\nS\tb\t333\t%s\tRC:i:1\nH\tVN:Z:2.0\n" % (a, b)
    cases["two headers, 2.0 then 1.1"] = b"H\tVN:Z:2.0\nS\ta\t400\t%s\nH\tVN:Z:1.1\n" % a
    cases["two headers, 1.0 then 2.0"] = b"H\tVN:Z:1.0\nS\ta\t400\t%s\nH\tzz:Z:q\tVN:Z:2.0\n" % a
    cases["header without VN"] = b"H\tfoo:Z:bar\n" + three + b"H\n"
    cases["paths before their segments"] = b"P\tp1\ta+,b-\t*\nP\tp2\tc+\t*\textra\ttabs\n" + three
    cases["path with semicolons"] = three + b"P\tp\ta+;b+;c-\t*\n"
    cases["path components without orientation"] = three + b"P\tp\ta,b+,cx,c+\t*\nP\tq\tb\t*\n"
    cases["path components naming no segment"] = three + b"P\tp\tzz+,a-,yy-\t*\nP\tq\tnone+\t*\n"
    cases["path whose ends are the same segment"] = three + b"P\tp\ta+\t*\nP\tq\tb-,b-\t*\n"
    cases["path lines that are no paths"] = three + b"P\nP\tp\nPX\tp\ta+\t*\nP\tok\tc-\n"
    cases["duplicate segment name"] = three + b"S\tb\tACGT\nS\ta\tACGT\n"
    cases["gfa2 with an E record"] = b"H\tVN:Z:2.0\nS\ta\t400\t%s\nS\tb\t333\t%s\nE\te1\ta+\tb+\t8\t8$\t0\t0\t0M\n" % (a, b)
    cases["gfa2 whose first foreign line is not its first"] = b"# c\nH\tVN:Z:2.0\n\nS\ta\t400\t%s\nGG\nE\te1\ta+\ta+\n" % a
    cases["gfa2 with a foreign first line"] = b"E\nS\ta\t4\tACGT\nH\tVN:Z:2.0\n"
    cases["L, W and C lines in a gfa1 input"] = b"H\tVN:Z:1.1\n" + three + b"L\ta\t+\tb\t+\t0M\nW\ts\t1\tchr\t0\t9\t>a<b\nC\ta\t+\tc\t+\t5\t9M\n"
    cases["pathless graph"] = b"H\tVN:Z:1.0\n" + three
    cases["a line of tabs"] = b"\t\t\t\n" + three
    cases["cr inside a line"] = b"S\ta\tAC\rGT\r\r\nS\tb\r\t%s\n" % b
    return cases


def crlf(text):
    return bytes(text).replace(b"\n", b"\r\n")


# -------------------------------------------------------------------------------------------- the library through ctypes
class Chunk(F.Chunk):
    """A ts_chunk fed with plain text or BGZF members, and the GFA stage over it."""

    def gfa_walk(self, at_end, seg_cap=1 << 12, line_cap=1 << 12, text_cap=1 << 16):
        """-> (rc, segments, lines, text, next, foreign, (*n_segs, *n_lines, *text_bytes)); what lies behind the entries and
        bytes taken must be as it was."""
        K = self.K
        segs, lines = (K.GfaSegment * (seg_cap + 1))(), (K.GfaLine * (line_cap + 1))()
        C.memset(segs, 0xEE, C.sizeof(segs))
        C.memset(lines, 0xEE, C.sizeof(lines))
        text = C.create_string_buffer(b"\xee" * (text_cap + 8), text_cap + 8)
        ns, nl, nb, nxt = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        fg = K.GfaForeign()
        rc = self.L.ts_gfa_chunk_walk(self.ptr, 1 if at_end else 0, segs, seg_cap, C.byref(ns), lines, line_cap, C.byref(nl), text,
                                      text_cap, C.byref(nb), C.byref(nxt), C.byref(fg))
        counts = (ns.value, nl.value, nb.value)
        foreign = (fg.off, fg.len) if fg.found else None
        if rc != K.TS_OK:
            return rc, [], [], b"", nxt.value, foreign, counts
        assert ns.value <= seg_cap and nl.value <= line_cap and nb.value <= text_cap
        got_segs = [(s.off, s.len, s.n_fields, s.f1_at, s.f1_len, s.f2_at, s.f2_len, s.f3_at, s.f3_len, s.name_at, s.star)
                    for s in segs[:ns.value]]
        got_lines = [(l.off, l.len, l.kind, l.text_at) for l in lines[:nl.value]]
        assert all(l.reserved == 0 for l in lines[:nl.value])
        rest = bytes(segs)[ns.value * C.sizeof(K.GfaSegment):]
        assert rest == b"\xee" * len(rest), "the walk wrote behind the segments it reported"
        rest = bytes(lines)[nl.value * C.sizeof(K.GfaLine):]
        assert rest == b"\xee" * len(rest), "the walk wrote behind the lines it reported"
        assert text.raw[nb.value:] == b"\xee" * (text_cap + 8 - nb.value), "the walk wrote behind the text it reported"
        return rc, got_segs, got_lines, text.raw[:nb.value], nxt.value, foreign, counts

    def data(self):
        return self.L.ts_chunk_data(self.ptr)

    def carry_over(self, source, carry_from, stream=None):
        """This chunk's contents become source's tail from carry_from; source must read back unchanged."""
        rc = self.L.ts_chunk_carry_over(self.ptr, source.ptr, carry_from, stream)
        assert rc == self.K.TS_OK, self.L.ts_last_error(self.ctx)
        self.mirror = source.mirror[carry_from:]
        assert self.size() == len(self.mirror) and self.read(0, len(self.mirror)) == self.mirror
        assert source.size() == len(source.mirror) and source.read(0, len(source.mirror)) == source.mirror
        return self.mirror
