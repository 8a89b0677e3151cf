"""FASTA body text for the TS_INPUT_TEXT_PIECES tests: the plain statement of "text to bases" (the one of
tests/cpp/text_pack_host.cpp), a renderer of sequences into lines, places to cut a text into pieces, and one call of
ts_scan_segments over segments of any mix of the four input formats.

A byte is a line end if it is LF, or if it is CR and the next byte is LF or it is the text's last byte; every other byte is a
base (a lone CR inside a line included: an invalid one)."""
import ctypes as C

WIDTHS = [1, 2, 31, 32, 33, 60, 63, 64, 65, 70, 80]
STYLES = ["lf", "crlf", "mix", "extras"]


def to_bases_bytewise(text):
    out = bytearray()
    for i, c in enumerate(text):
        if c == 10 or (c == 13 and (i + 1 == len(text) or text[i + 1] == 10)):
            continue
        out.append(c)
    return bytes(out)


def to_bases(text):
    """The same for long texts: a CR in front of an LF goes with it (one pass, left to right, so of CR CR LF the first CR stays),
    a CR at the very end goes, every LF goes."""
    t = text.replace(b"\r\n", b"\n")
    if t.endswith(b"\r"):
        t = t[:-1]
    return t.replace(b"\n", b"")


def render(seq, width, style, rng, first=None, ending=None):
    """seq in lines of `width` bases (the first of `first`), ending in LF ("lf"), CRLF ("crlf"), either ("mix"), or either with now
    and then a blank line, CR CR LF, or a lone CR inside a line ("extras": these CRs are bases, so to_bases(text) is longer than
    seq).  ending: what follows the last base — b"", b"\\n", b"\\r\\n" or b"\\r" (drawn if None)."""
    out, at, limit = [], 0, first or width
    n = len(seq)
    while at < n:
        line = seq[at:at + limit]
        at += len(line)
        limit = width
        if style == "extras" and len(line) > 2 and rng.random() < 0.02:
            k = int(rng.integers(1, len(line) - 1))
            line = line[:k] + b"\r" + line[k:]
        out.append(line)
        if at >= n:
            break
        crlf = style == "crlf" or (style in ("mix", "extras") and rng.random() < 0.5)
        end = b"\r\n" if crlf else b"\n"
        if style == "extras":
            r = rng.random()
            if r < 0.02:
                end = b"\r\r\n"
            elif r < 0.05:
                end = end + end
        out.append(end)
    if ending is None:
        ending = [b"", b"\n", b"\r\n", b"\r"][int(rng.integers(0, 4))]
    return b"".join(out) + ending


def cut_places(text, rng, n, near=()):
    """Up to n byte positions to cut `text` at, of four kinds in turn: inside a line, right before a line end, between a CR and
    its LF, right behind an LF — and one inside a line next to each base index of `near` that allows it.  Never right behind a CR
    that is a base (at the end of a piece it would read as a line end)."""
    lf = [i for i in range(len(text)) if text[i] == 10]
    crlf = [i for i in lf if i and text[i - 1] == 13]
    cuts = set()
    for k in range(n):
        kind = k % 4
        if kind == 0:
            p = int(rng.integers(1, len(text)))
        elif kind == 1 and lf:
            p = lf[int(rng.integers(0, len(lf)))]
            if p and text[p - 1] == 13:
                p -= 1
        elif kind == 2 and crlf:
            p = crlf[int(rng.integers(0, len(crlf)))]
        elif lf:
            p = lf[int(rng.integers(0, len(lf)))] + 1
        else:
            continue
        cuts.add(p)
    if near:
        # base index -> text index, by walking the text once
        want, at, b = sorted(near), 0, 0
        for i, c in enumerate(text):
            if at >= len(want):
                break
            if c == 10 or (c == 13 and (i + 1 == len(text) or text[i + 1] == 10)):
                continue
            if b == want[at]:
                cuts.add(i)
                at += 1
            b += 1
    ok = sorted(p for p in cuts if 0 < p < len(text) and not (text[p - 1] == 13 and text[p] != 10))
    return ok


def behind_bases(text, k):
    """(p, b): a text position p at a base, with b >= k bases in front of it (bisection over to_bases of the prefixes)."""
    lo, hi = 0, len(text)
    while lo < hi:
        mid = (lo + hi) // 2
        if len(to_bases(text[:mid] + b"A")) - 1 >= k:
            hi = mid
        else:
            lo = mid + 1
    while lo < len(text) and text[lo] in b"\r\n":
        lo += 1
    return lo, len(to_bases(text)) - len(to_bases(text[lo:]))


def split(text, cuts):
    """The text's pieces; the pieces' bases, joined, are the text's (asserted: the rule is applied per piece)."""
    edges = [0] + list(cuts) + [len(text)]
    blobs = [text[a:b] for a, b in zip(edges, edges[1:])]
    assert b"".join(to_bases(b) for b in blobs) == to_bases(text)
    return blobs


def text_pieces(K, blobs):
    arr = (K.TextPiece * max(1, len(blobs)))()
    for i, bl in enumerate(blobs):
        arr[i].text, arr[i].text_len, arr[i].n_bases = bl, len(bl), len(to_bases(bl))
    return arr


def scan_call(tel, entries, device_bytes=None, raw=False):
    """One ts_scan_segments call.  entries: [(format, payload, abs_pos, tips)] — payload: the bases (TS_INPUT_BASES,
    TS_INPUT_PACKED2: packed here with the context's case folding, TS_INPUT_DEVICE: copied to the device by device_bytes(bytes))
    or the list of a text's pieces (TS_INPUT_TEXT_PIECES; a (blobs, declared length, piece array) triple to declare something
    else than the pieces hold).  -> [segment dicts], or the return code when raw."""
    import teloscope_amd as ta
    from teloscope_amd import _capi as K
    from tests.backends import segment_as_dict
    n = len(entries)
    arr, keep, on_device = (K.SegmentIn * max(1, n))(), [], []
    for i, (fmt, payload, abs_pos, tips) in enumerate(entries):
        if fmt == K.TS_INPUT_TEXT_PIECES:
            if isinstance(payload, tuple):
                blobs, length, pieces = payload
            else:
                blobs, pieces = payload, text_pieces(K, payload)
                length = sum(int(p.n_bases) for p in pieces[:len(blobs)])
            keep.append((blobs, pieces))
            arr[i].seq, arr[i].n_pieces = C.cast(pieces, C.c_char_p), len(blobs)
        elif fmt == K.TS_INPUT_PACKED2:
            ps, alive = K.pack_sequence(payload, tel.userInput.foldCase)
            keep.append((payload, ps, alive))
            arr[i].seq, length = C.cast(C.pointer(ps), C.c_char_p), len(payload)
        elif fmt == K.TS_INPUT_DEVICE:
            d = device_bytes(payload)
            on_device.append(d)
            arr[i].seq, length = d.ptr, len(payload)
        else:
            keep.append(payload)
            arr[i].seq, length = payload, len(payload)
        arr[i].len, arr[i].abs_pos, arr[i].tips_only, arr[i].input_format = length, abs_pos, int(tips), fmt
    out = (K.SegmentOut * max(1, n))()
    try:
        rc = K.lib().ts_scan_segments(tel._ctx.ptr, arr, n, out)
        if raw:
            if rc == K.TS_OK:
                K.lib().ts_free_segments(out, n)
            return rc
        assert rc == K.TS_OK, tel._ctx.error()
        res = [segment_as_dict(ta.SegmentData(out[i], bool(entries[i][3]))) for i in range(n)]
        K.lib().ts_free_segments(out, n)
        return res
    finally:
        for d in on_device:
            d.free()
