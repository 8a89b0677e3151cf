"""Handmade raw deflate streams (RFC 1951) for the tests of the inflate core and of the BGZF kernel: a bit writer that emits
any token sequence and any code-length set, valid or not, and the named, seeded case lists built with it.  No tests in here.

A token is a literal byte (an int), a match (length, distance), or one of three raw forms that only broken members use:
("lsym", s) and ("dsym", s) write symbol s of the block's literal/length or distance code without extra bits, ("bits", v, n)
writes n bits as they are.  expand() is what the tokens mean; zlib's decoder (zlib_verdict of tests/test_inflate_core_cpu.py)
judges every case when its list is built: the accepted lists are accepted with expand()'s bytes, the rejected members of
tables_bad are rejected.  The decoder under test has no say in that.

cases(name) -> [(tag, payload, isize, crc)], plains(name) -> {tag: bytes} for the members zlib accepts.
Lists: match_grid, chains, big_batches, blocks, tables_ok (accepted), tables_bad (one rule broken per member, and the few
valid neighbours its tags name), crc_grid (stored members of 0..130 bytes)."""
import functools
import random
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [x for x in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
ACCEPTED = ("match_grid", "chains", "big_batches", "blocks", "tables_ok")
OK, BAD_DEFLATE = 0, 1


def length_symbol(n):
    """(symbol, extra bits, their value) of a match length 3..258"""
    assert 3 <= n <= 258
    i = 28 if n == 258 else max(k for k in range(28) if LEN_BASE[k] <= n)
    return 257 + i, LEN_EXTRA[i], n - LEN_BASE[i]


def dist_symbol(d):
    assert 1 <= d <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    return i, DIST_EXTRA[i], d - DIST_BASE[i]


def canonical_codes(lens):
    """RFC 1951's code assignment for any lengths (an over-subscribed set's codes wrap, as its counts say)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append(nxt[l] & ((1 << l) - 1) if l else None)
        nxt[l] += 1 if l else 0
    return out


def kraft(lens):
    """sum of 2^-len over the codes, in units of 2^-15: 32768 is a complete set"""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lengths(k, rng, maxbits, deep=False):
    """k >= 2 code lengths of a complete prefix code, none above maxbits: leaves split at random (rng None: the shallowest
    first), from a staircase 1, 2, .. d, d that reaches maxbits where deep is set.  Shuffled when rng is given."""
    assert 2 <= k <= 1 << maxbits
    d = min(maxbits, k - 1) if deep else 1
    leaves = list(range(1, d + 1)) + [d]
    while len(leaves) < k:
        open_ = [i for i, l in enumerate(leaves) if l < maxbits]
        i = rng.choice(open_) if rng else min(open_, key=lambda j: leaves[j])
        leaves[i] += 1
        leaves.append(leaves[i])
    if rng:
        rng.shuffle(leaves)
    assert kraft(leaves) == 32768
    return leaves


def cl_sequence(lens, mode="greedy"):
    """The code-length symbols that send `lens` (literal/length and distance lengths as one run, which is how a repeat
    crosses from one to the other): [(symbol, extra value, first index, count)].  mode "none" uses no repeat code,
    "greedy" the longest repeat at every point, "zeros16" ends every run of zeros that 17 / 18 began with a 16."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, run = lens[i], 1
        while i + run < n and lens[i + run] == v:
            run += 1
        if mode == "none":
            out.append((v, 0, i, 1)); i += 1
        elif v == 0 and run >= 3:
            take = min(run, 138)
            if mode == "zeros16" and run >= 6:
                take = min(run - 3, 138)
            out.append((17, take - 3, i, take) if take <= 10 else (18, take - 11, i, take)); i += take
            if mode == "zeros16" and run - take >= 3:
                rep = min(run - take, 6)
                out.append((16, rep - 3, i, rep)); i += rep
        elif v != 0 and run >= 4:
            out.append((v, 0, i, 1)); i += 1
            left = run - 1
            while left >= 3:
                rep = min(left, 6)
                out.append((16, rep - 3, i, rep)); i += rep; left -= rep
        else:
            out.append((v, 0, i, 1)); i += 1
    return out


def default_clens(symbols, rng=None, deep=False):
    """A complete code-length code (19 lengths, none above 7) over the given code-length symbols."""
    used = sorted(set(symbols))
    if len(used) == 1:
        used.append(next(s for s in (0, 1, 2) if s != used[0]))   # (zlib takes no incomplete code-length code, one code included)
    ls = complete_lengths(len(used), rng, 7, deep)
    clens = [0] * 19
    for s, l in zip(used, ls):
        clens[s] = l
    return clens


def expand(tokens, before=b""):
    """The bytes the tokens stand for, behind `before` (which matches may reach into); raw tokens stand for nothing."""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif not isinstance(t[0], str):
            n, d = t
            assert 1 <= d <= len(out), (t, len(out))
            for _ in range(n):
                out.append(out[-d])
    return bytes(out[len(before):])


class Stream:
    """The bit writer: LSB-first, Huffman codes with their first bit first (that is, bit-reversed)."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        assert 0 <= v < 1 << n
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def nbits(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        """the stream so far, its last byte padded with zero bits"""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")

    def stored_block(self, data, last, nlen=None):
        assert len(data) <= 65535
        self.bits(1 if last else 0, 1); self.bits(0, 2)
        if self.n:
            self.bits(0, 8 - self.n)
        self.bits(len(data), 16)
        self.bits(len(data) ^ 0xffff if nlen is None else nlen, 16)
        self.out += data

    def _tokens(self, tokens, lit_lens, dist_lens, eob):
        lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
        for t in tokens:
            if isinstance(t, int):
                self.code(lc[t], lit_lens[t])
            elif t[0] == "bits":
                self.bits(t[1], t[2])
            elif t[0] == "lsym":
                self.code(lc[t[1]], lit_lens[t[1]])
            elif t[0] == "dsym":
                self.code(dc[t[1]], dist_lens[t[1]])
            else:
                s, xb, xv = length_symbol(t[0])
                self.code(lc[s], lit_lens[s]); self.bits(xv, xb)
                s, xb, xv = dist_symbol(t[1])
                self.code(dc[s], dist_lens[s]); self.bits(xv, xb)
        if eob:
            self.code(lc[256], lit_lens[256])

    def fixed_block(self, tokens, last, eob=True):
        self.bits(1 if last else 0, 1); self.bits(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST, eob)

    def dynamic_block(self, tokens, lit_lens, dist_lens, last, clens=None, rle="greedy", hclen=None, eob=True):
        """The header says what it is given, valid or not: HLIT = len(lit_lens) - 257 (257..288), HDIST = len(dist_lens) - 1
        (1..32), the code-length symbols of `rle` (a mode of cl_sequence, or a list of (symbol, extra value, ...) sent as it
        is, whatever the lengths are), coded by `clens` (default: a complete code over the symbols sent), of which `hclen`
        (default: as many as are not zero, 4 at least) are written.  The data is coded by lit_lens and dist_lens."""
        assert 257 <= len(lit_lens) <= 288 and 1 <= len(dist_lens) <= 32
        seq = cl_sequence(list(lit_lens) + list(dist_lens), rle) if isinstance(rle, str) else rle
        if clens is None:
            clens = default_clens([s[0] for s in seq])
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if clens[CL_ORDER[i]]])
        assert 4 <= hclen <= 19
        self.bits(1 if last else 0, 1); self.bits(2, 2)
        self.bits(len(lit_lens) - 257, 5); self.bits(len(dist_lens) - 1, 5); self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(clens[CL_ORDER[i]], 3)
        cc = canonical_codes(clens)
        for s in seq:
            self.code(cc[s[0]], clens[s[0]])
            if s[0] >= 16:
                self.bits(s[1], {16: 2, 17: 3, 18: 7}[s[0]])
        self._tokens(tokens, lit_lens, dist_lens, eob)


# ------------------------------------------------------------------------------------------------ tokens and tables at random
SOUP_LENGTHS = (3, 4, 5, 8, 17, 63, 64, 65, 258, None)             # None: any of 3..258


def soup(rng, size, before=0, alphabet=b"ACGT", near=0.9, p_match=0.5, lengths=SOUP_LENGTHS, reach=70):
    """Tokens for exactly `size` bytes behind `before` earlier ones: literals of the alphabet and matches, `near` of whose
    distances are at most `reach` (all of them while no more bytes than that lie behind)."""
    tokens, made = [], 0
    while made < size:
        pos, left = before + made, size - made
        if pos > 0 and left >= 3 and rng.random() < p_match:
            n = rng.choice(lengths)
            n = min(left, rng.randint(3, 258) if n is None else n)
            d = rng.randint(1, min(reach, pos)) if pos <= reach or rng.random() < near else rng.randint(reach + 1, pos)
            tokens.append((n, d)); made += n
        else:
            tokens.append(rng.choice(alphabet)); made += 1
    return tokens


def symbols_used(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        elif not isinstance(t[0], str):
            lit.add(length_symbol(t[0])[0]); dist.add(dist_symbol(t[1])[0])
    return lit, dist


def tables_for(tokens, rng, maxbits=15, unused=0, deep=False, nl=None, nd=None):
    """Random complete literal/length and distance sets under which the tokens can be written: over the symbols they use
    and `unused` more of each kind.  No distance symbol: one zero length; one: the single one-bit code."""
    lit, dist = symbols_used(tokens)
    lit |= set(rng.sample([s for s in range(286) if s not in lit], min(unused, 286 - len(lit))))
    dist |= set(rng.sample([s for s in range(30) if s not in dist], min(unused, 30 - len(dist))))
    if len(lit) == 1:
        lit.add(rng.randrange(256))
    lit, dist = sorted(lit), sorted(dist)
    lit_lens = [0] * (nl or max(257, lit[-1] + 1))
    for s, l in zip(lit, complete_lengths(len(lit), rng, maxbits, deep)):
        lit_lens[s] = l
    dist_lens = [0] * (nd or (dist[-1] + 1 if dist else 1))
    if len(dist) == 1:
        dist_lens[dist[0]] = 1
    elif dist:
        for s, l in zip(dist, complete_lengths(len(dist), rng, maxbits, deep)):
            dist_lens[s] = l
    return lit_lens, dist_lens


def flush_profile(blocks):
    """What the kernel's flush meets in a member, counted from the tokens as the core batches them (64 symbols to a batch;
    a stored block and the member's end flush a partial one; a batch may span fixed and dynamic blocks).  blocks:
    [("stored", data) | ("fixed" | "dynamic", tokens, ...)].  -> dict: batches, the most bytes of one, matches with a byte
    whose source is a byte of another match written in the same 64-byte group (chained), the longest run of such hops
    from a byte to a literal or to a byte of an earlier group (depth), matches that start in one group and end in another."""
    prof = dict(batches=0, max_bytes=0, chained=0, depth=0, crossing=0, batch_sizes=set())
    batch = []

    def flush():
        if not batch:
            return
        owner, start = [], []
        for k, t in enumerate(batch):
            start.append(len(owner))
            owner += [k] * (1 if isinstance(t, int) else t[0])
        depth = [0] * len(owner)
        chained = set()
        for b, k in enumerate(owner):
            t = batch[k]
            if isinstance(t, int):
                continue
            src = start[k] - t[1] + (b - start[k]) % t[1]
            if src >= b - b % 64:
                depth[b] = 1 + depth[src]
                if not isinstance(batch[owner[src]], int):
                    chained.add(k)
        prof["batches"] += 1
        prof["batch_sizes"].add(len(batch))
        prof["max_bytes"] = max(prof["max_bytes"], len(owner))
        prof["chained"] += len(chained)
        prof["depth"] = max([prof["depth"]] + depth)
        prof["crossing"] += sum(1 for k, t in enumerate(batch) if not isinstance(t, int) and start[k] // 64 != (start[k] + t[0] - 1) // 64)
        del batch[:]

    for blk in blocks:
        if blk[0] == "stored":
            flush()
            continue
        for t in blk[1]:
            if isinstance(t, int) or not isinstance(t[0], str):
                batch.append(t)
                if len(batch) == 64:
                    flush()
    flush()
    return prof


def member(blocks):
    """blocks: [("stored", data) | ("fixed", tokens) | ("dynamic", tokens, keywords of dynamic_block)], the last one final.
    -> (payload, the bytes they stand for, the Stream)"""
    s, plain = Stream(), b""
    for i, blk in enumerate(blocks):
        last = i == len(blocks) - 1
        if blk[0] == "stored":
            s.stored_block(blk[1], last); plain += blk[1]
        else:
            if blk[0] == "fixed":
                s.fixed_block(blk[1], last)
            else:
                s.dynamic_block(blk[1], last=last, **blk[2])
            plain += expand(blk[1], plain)
    return s.bytes(), plain, s


def crc_of(data):
    return zlib.crc32(data) & 0xFFFFFFFF


class _List:
    def __init__(self):
        self.cases, self.plains, self.rejected = [], {}, set()

    def ok(self, tag, payload, plain):
        assert tag not in self.plains and tag not in self.rejected, tag
        assert len(payload) <= 65536 and len(plain) <= 65536, tag
        self.cases.append((tag, payload, len(plain), crc_of(plain)))
        self.plains[tag] = plain

    def blocks(self, tag, blocks):
        payload, plain, s = member(blocks)
        self.ok(tag, payload, plain)
        return s

    def bad(self, tag, payload, isize, crc=0):
        assert tag not in self.plains and tag not in self.rejected, tag
        assert len(payload) <= 65536 and isize <= 65536, tag
        self.cases.append((tag, payload, isize, crc))
        self.rejected.add(tag)


# ---------------------------------------------------------------------------------------------------------------- the lists
GRID_P = (0, 1, 2, 31, 62, 63, 64, 65)
GRID_DIST = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129)
GRID_FAR = (32767, 32768)
GRID_LEN = (3, 4, 5, 61, 62, 63, 64, 65, 66, 127, 128, 129, 257, 258)


def _match_grid():
    """Fixed codes, one match per member: 64 m literals (whole batches; the fewest that put the distance inside the member),
    p literals, the match, a literal.  The far distances read a stored block of 32 768 bytes instead."""
    rng, L = random.Random(1001), _List()
    far = bytes(rng.getrandbits(8) for _ in range(32768))
    for p in GRID_P:
        dists = sorted(set(GRID_DIST) | {d for d in (p, p + 1, p + 63, p + 64, p + 65) if d >= 1})
        for d in dists:
            m = max(0, -(-(d - p) // 64))
            for n in GRID_LEN:
                tokens = [rng.getrandbits(8) for _ in range(64 * m + p)] + [(n, d), rng.getrandbits(8)]
                L.blocks("grid:p%d:d%d:n%d" % (p, d, n), [("fixed", tokens)])
        for d in GRID_FAR:
            for n in GRID_LEN:
                tokens = [rng.getrandbits(8) for _ in range(p)] + [(n, d), rng.getrandbits(8)]
                L.blocks("grid:far:p%d:d%d:n%d" % (p, d, n), [("stored", far), ("fixed", tokens)])
    return L


CHAIN_SIZES = (1, 63, 64, 65, 200, 5000, 20000)


def _chains():
    """Token soups over four letters, fixed and dynamic codes in turn; every third one has short matches at short distances
    only, and ladders (the same short match over and over, each one copying the one before) end the list.  What the list is
    for is counted, not assumed: most distances are at most 70, and there are matches whose source is another match of the
    same 64-byte group, in chains of more than 16 hops: the pointer jumping between lanes needs all its rounds but one."""
    rng, L = random.Random(1002), _List()
    near = far = 0
    total = dict(chained=0, depth=0, crossing=0, max_bytes=0)
    for size in CHAIN_SIZES:
        for k in range(24):
            tokens = soup(rng, size, lengths=(3, 3, 4, 5), reach=6, p_match=0.7) if k % 3 == 2 else soup(rng, size)
            if k % 2:
                lit_lens, dist_lens = tables_for(tokens, rng)
                blocks = [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens))]
            else:
                blocks = [("fixed", tokens)]
            L.blocks("chains:%d:%d" % (size, k), blocks)
            prof = flush_profile(blocks)
            for key in ("chained", "crossing"):
                total[key] += prof[key]
            for key in ("depth", "max_bytes"):
                total[key] = max(total[key], prof[key])
            for t in tokens:
                if not isinstance(t, int):
                    near += t[1] <= 70
                    far += t[1] > 70
    for d in (1, 2, 3, 4):
        for n in (3, 4, 5):
            blocks = [("fixed", [rng.choice(b"ACGT") for _ in range(d)] + [(n, d)] * 40)]
            L.blocks("chains:ladder:d%d:n%d" % (d, n), blocks)
            total["depth"] = max(total["depth"], flush_profile(blocks)["depth"])
    L.profile = dict(total, near=near, far=far)
    assert near >= 0.9 * (near + far) and far >= 0.03 * (near + far), (near, far)
    assert total["chained"] >= 1000 and total["depth"] > 16 and total["crossing"] >= 1000 and total["max_bytes"] > 1024, total
    return L


def _big_batches():
    """64 and 65 matches of 258 in a row (one flush writes 16 512 bytes) behind whole batches of literals or behind a stored
    block, and batches of 63, 64 and 65 symbols that the end-of-block code follows at once."""
    rng, L = random.Random(1003), _List()
    for d in (1, 2, 63, 64, 65, 258, 259):
        for count in (64, 65):
            lits = [rng.choice(b"ACGT") for _ in range(64 * -(-d // 64))]
            blocks = [("fixed", lits + [(258, d)] * count)]
            L.blocks("big:lit:d%d:x%d" % (d, count), blocks)
            assert flush_profile(blocks)["max_bytes"] == 16512
            blocks = [("stored", bytes(rng.choice(b"ACGT") for _ in range(d))), ("fixed", [(258, d)] * count)]
            L.blocks("big:stored:d%d:x%d" % (d, count), blocks)
            assert flush_profile(blocks)["max_bytes"] == 16512
    for count in (63, 64, 65):
        for k in range(6):
            tokens = [rng.choice(b"ACGT")]
            while len(tokens) < count:
                pos = len(expand(tokens))
                tokens.append(rng.choice(b"ACGT") if rng.random() < 0.4 else (rng.choice((3, 4, 5, 64, 258)), rng.randint(1, min(pos, 70))))
            for more in ("", "+stored", "+fixed"):
                blocks = [("fixed", tokens)] + {"": [], "+stored": [("stored", b"TTAGGG")], "+fixed": [("fixed", [(9, 3), 65])]}[more]
                L.blocks("big:end%d:%d%s" % (count, k, more), blocks)
                if not more:
                    assert flush_profile(blocks)["batch_sizes"] == {63: {63}, 64: {64}, 65: {64, 1}}[count]
    return L


def _blocks():
    """Members of 2..8 blocks of the three types: every order of two and three, orders at random beyond; matches reach into
    the blocks before; empty stored blocks; a partial batch that a stored block flushes; final blocks that end 0..7 bits
    before a byte boundary; the empty dynamic block whose literal/length set is the one-bit end-of-block code alone."""
    rng, L = random.Random(1004), _List()

    def block(kind, before):
        if kind == "stored":
            return ("stored", bytes(rng.choice(b"ACGT") for _ in range(rng.choice((0, 0, 1, 5, 64, 100)))))
        tokens = soup(rng, rng.choice((0, 1, 3, 40, 64, 130, 300)), before)
        if kind == "fixed":
            return ("fixed", tokens)
        lit_lens, dist_lens = tables_for(tokens, rng)
        return ("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens, rle=rng.choice(("greedy", "none", "zeros16"))))

    def build(tag, kinds):
        blocks, before = [], 0
        for kind in kinds:
            blocks.append(block(kind, before))
            before += len(blocks[-1][1]) if kind == "stored" else len(expand(blocks[-1][1], b"\0" * before))
        L.blocks(tag, blocks)

    kinds3 = ("stored", "fixed", "dynamic")
    orders = [(a, b) for a in kinds3 for b in kinds3] + [(a, b, c) for a in kinds3 for b in kinds3 for c in kinds3]
    for n in range(4, 9):
        orders += [tuple(rng.choice(kinds3) for _ in range(n)) for _ in range(16)]
    for i, kinds in enumerate(orders):
        build("blocks:%d:%s" % (i, "".join(k[0] for k in kinds)), kinds)
    # what Z_SYNC_FLUSH leaves: an empty stored block behind a block that is not the last
    for k in range(8):
        a, b = soup(rng, 100 + k), None
        b = soup(rng, 150, 100 + k)
        la, da = tables_for(a, rng)
        first = ("dynamic", a, dict(lit_lens=la, dist_lens=da)) if k % 2 else ("fixed", a)
        L.blocks("blocks:sync:%d" % k, [first] + [("stored", b"")] * (1 + k % 3) + [("fixed", b)] + ([("stored", b"")] if k >= 4 else []))
    # a batch of p symbols that a stored block flushes, then matches into both
    for p in (1, 2, 63, 64, 65, 100):
        a = [rng.choice(b"ACGT") for _ in range(3)] + [(4, 2)] * (p - 3) if p > 3 else [rng.choice(b"ACGT")] * p
        na = len(expand(a))
        mid = bytes(rng.choice(b"ACGT") for _ in range(37))
        b = [(20, 37 + na), (30, 50), rng.choice(b"ACGT"), (258, min(70, na + 37))]
        L.blocks("blocks:partial:p%d" % p, [("fixed", a), ("stored", mid), ("fixed", b)])
    # padding bits behind the final end-of-block code: 3 + 8 a + 9 b + 7 bits in all
    pads = set()
    for b9 in range(8):
        s = L.blocks("blocks:pad:%d" % b9, [("fixed", [65, 67] + [200 + b9] * b9)])
        pads.add(-s.nbits() % 8)
    assert pads == set(range(8)), pads
    one_bit = [0] * 256 + [1]
    L.blocks("blocks:empty_dynamic", [("dynamic", [], dict(lit_lens=one_bit, dist_lens=[0]))])
    L.blocks("blocks:empty_dynamic_behind", [("fixed", soup(rng, 70)), ("dynamic", [], dict(lit_lens=one_bit, dist_lens=[0]))])
    L.blocks("blocks:empty_fixed", [("fixed", [])])
    L.blocks("blocks:empty_stored", [("stored", b"")])
    return L


def code_lengths_in_use(tokens, lit_lens, dist_lens):
    lit, dist = set(), set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(lit_lens[t])
        elif not isinstance(t[0], str):
            lit.add(lit_lens[length_symbol(t[0])[0]]); dist.add(dist_lens[dist_symbol(t[1])[0]])
    return lit, dist


def _tables_ok():
    rng, L = random.Random(1005), _List()
    # codes beyond the lookups (10 / 8 / 7 bits), met in the data: a staircase 1, 2, .. 15, 15 over 16 symbols of each kind,
    # turned so that every symbol gets every length; and random sets over many symbols
    slow_lit, slow_dist = set(), set()
    lit_syms = [65, 67, 71, 84, 0, 255, 143, 144, 256, 257, 258, 264, 265, 284, 285, 10]
    dist_syms = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]
    stairs = list(range(1, 16)) + [15]
    for turn in range(16):
        lit_lens, dist_lens = [0] * 286, [0] * 18
        for i, s in enumerate(lit_syms):
            lit_lens[s] = stairs[(i + turn) % 16]
        for i, s in enumerate(dist_syms):
            dist_lens[s] = stairs[(i + turn) % 16]
        tokens = [rng.choice((65, 67, 71, 84, 0, 255, 143, 144, 10)) for _ in range(300)]
        for _ in range(60):
            pos = len(expand(tokens))
            n = rng.choice((3, 4, 10, 11, 12, 227, 230, 257, 258))
            d = rng.choice([x for x in (1, 2, 3, 4, 5, 6, 7, 8, 17, 24, 33, 48, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 300, 384) if x <= pos])
            tokens += [(n, d), rng.choice((65, 67, 71, 84, 0, 255, 143, 144, 10))]
        a, b = code_lengths_in_use(tokens, lit_lens, dist_lens)
        slow_lit |= a; slow_dist |= b
        L.blocks("ok:stairs:%d" % turn, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens, rle=("greedy", "none")[turn % 2]))])
    assert slow_lit >= set(range(1, 16)) and slow_dist >= set(range(1, 16))
    slow_lit, slow_dist = set(), set()
    for k in range(40):
        tokens = soup(rng, 3000, alphabet=bytes(range(256)), near=0.5, p_match=0.3)
        lit_lens, dist_lens = tables_for(tokens, rng, unused=rng.choice((0, 5, 40)), deep=True)
        a, b = code_lengths_in_use(tokens, lit_lens, dist_lens)
        slow_lit |= a; slow_dist |= b
        L.blocks("ok:random:%d" % k, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens, rle=rng.choice(("greedy", "none", "zeros16"))))])
    assert slow_lit >= set(range(11, 16)) and slow_dist >= set(range(11, 16)), (slow_lit, slow_dist)
    # a code-length code with 7-bit codes, all 19 of its lengths sent (lengths 1..15 and the three repeat codes all in use)
    for k in range(8):
        tokens = soup(rng, 2000, alphabet=bytes(range(256)), near=0.5, p_match=0.3)
        lit_lens, dist_lens = tables_for(tokens, rng, unused=30, deep=True, nl=286, nd=30)
        seq = cl_sequence(lit_lens + dist_lens, "greedy")
        used = {s[0] for s in seq}
        clens = default_clens(used | set(range(19)) if k % 2 else used, rng, deep=True)
        assert max(clens) == 7
        hclen = 19 if k % 2 else None
        L.blocks("ok:clen7:%d" % k, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens, rle=seq, clens=clens, hclen=hclen))])
    # the fewest code-length lengths a valid block can send: 16, 17, 18, 0 and 8 (HCLEN 5; with four, no length but zero can
    # be said, and the end-of-block code has none: that one is in tables_bad).  255 literals and 256, all of eight bits.
    lit_lens = [8] * 257
    lit_lens[255] = 0
    for mode in ("none", "greedy"):
        tokens = [rng.randrange(255) for _ in range(500)]
        s = L.blocks("ok:hclen5:" + mode, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=[0], rle=mode, hclen=5,
                                                                  clens=default_clens([0, 8] + ([16, 17] if mode == "greedy" else []))))])
    # HLIT 257 with HDIST 1 and no distance code; one distance code of one bit; HLIT 286 with HDIST 30
    for k in range(4):
        tokens = [rng.choice(b"ACGTN\n") for _ in range(200)]
        lit_lens, dist_lens = tables_for(tokens, rng)
        assert len(lit_lens) == 257 and dist_lens == [0]
        L.blocks("ok:hlit257:%d" % k, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens))])
    for k, d in enumerate((1, 2, 3, 4, 7, 100)):
        tokens = [rng.choice(b"ACGT") for _ in range(140)]
        for _ in range(50):
            x = dist_symbol(d)
            tokens += [(rng.choice((3, 5, 64, 258)), DIST_BASE[x[0]] + rng.randrange(1 << x[1])), rng.choice(b"ACGT")]
        lit_lens, dist_lens = tables_for(tokens, rng)
        assert sorted(dist_lens)[-2:] == ([1] if len(dist_lens) == 1 else [0, 1])
        L.blocks("ok:one_dist:%d" % k, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens))])
    for k in range(4):
        tokens = soup(rng, 4000, alphabet=bytes(range(256)), near=0.3, p_match=0.5)
        lit_lens, dist_lens = tables_for(tokens, rng, unused=300, nl=286, nd=30)
        assert 0 not in lit_lens and 0 not in dist_lens
        L.blocks("ok:full:%d" % k, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens, rle=("greedy", "none")[k % 2]))])
    # 16 across the boundary between the two sets; 18 with 138 zeros; 16 straight behind 17 and 18 (it repeats zero)
    for k in range(4):
        tokens = [rng.choice(b"ACGT") for _ in range(80)] + [(3 + k, 1 + k), 65, (258, 2 + k), 67, (17, 3)]
        lit, dist = symbols_used(tokens)
        lit, dist = lit | {283, 284, 285}, dist | {0, 1, 2}
        lit |= set(range(100, 100 + 16 - len(lit)))                 # 16 symbols of each kind: every code has four bits
        dist |= set(range(10, 10 + 16 - len(dist)))
        lit_lens, dist_lens = [4 * (s in lit) for s in range(286)], [4 * (s in dist) for s in range(max(dist) + 1)]
        seq = cl_sequence(lit_lens + dist_lens, "greedy")
        assert any(s[0] == 16 and s[2] < 286 < s[2] + s[3] for s in seq), seq
        L.blocks("ok:16_across:%d" % k, [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens, rle=seq))])
    for k, mode in enumerate(("greedy", "zeros16", "greedy", "zeros16")):
        tokens = [rng.choice((1 + k, 2, 240, 250, 251)) for _ in range(100)] + [(3, 1), (258, 2)]
        lit_lens, dist_lens = tables_for(tokens, rng)
        seq = cl_sequence(lit_lens + dist_lens, mode)
        assert any(s[0] == 18 and s[1] == 127 for s in seq), seq
        if mode == "zeros16":
            for first in (17, 18):
                assert any(a[0] == first and b[0] == 16 for a, b in zip(seq, seq[1:])), (first, seq)
        L.blocks("ok:zeros:%s:%d" % (mode, k), [("dynamic", tokens, dict(lit_lens=lit_lens, dist_lens=dist_lens, rle=seq))])
    # 258 as symbol 284 with all its extra bits set, which zlib takes
    L.blocks("ok:258_as_284", [("fixed", [65, 66, ("lsym", 284), ("bits", 31, 5), ("dsym", 1), 67])])
    L.plains["ok:258_as_284"] = b"AB" + b"AB" * 129 + b"C"
    L.cases[-1] = ("ok:258_as_284", L.cases[-1][1], 261, crc_of(L.plains["ok:258_as_284"]))
    return L


BAD_RULES = ("over:lit", "over:dist", "over:clen", "longer:lit", "longer:dist", "longer:clen", "dropped:lit", "dropped:dist",
             "dropped:clen", "first16", "past_end", "eob0", "hlit287", "hlit288", "hdist31", "hdist32", "hclen4", "unused",
             "sym286", "sym287", "dsym30", "dsym31", "dist_pos+1", "more:lit", "more:match", "fewer:lit", "fewer:match",
             "trail", "type3", "nlen")
BAD_VALID = ("dist_pos", "control")                                  # tags of tables_bad that zlib accepts


def _tables_bad():
    """One rule broken per member; tag = "bad:<rule>:...", the rules of BAD_RULES.  The members tagged with BAD_VALID are the
    valid neighbours: a distance of exactly the bytes written, and the unbroken member that the others are made from."""
    rng, L = random.Random(1006), _List()

    def dyn(tag, tokens, lit_lens, dist_lens, valid=False, **kw):
        s = Stream()
        s.dynamic_block(tokens, lit_lens, dist_lens, True, **kw)
        plain = expand(tokens)
        if valid:
            L.ok(tag, s.bytes(), plain)
        else:
            L.bad(tag, s.bytes(), len(plain), crc_of(plain))

    for k in range(12):
        tokens = soup(rng, 400, alphabet=b"ACGTN\n", near=0.6)
        while len(symbols_used(tokens)[1]) < 3:
            tokens = soup(rng, 400, alphabet=b"ACGTN\n", near=0.6)
        lit_lens, dist_lens = tables_for(tokens, rng, unused=3)
        both = lit_lens + dist_lens
        mode = ("greedy", "none", "zeros16")[k % 3]
        seq = cl_sequence(both, mode)
        spare = next(s for s in range(1, 16) if s not in both)
        clens = default_clens({s[0] for s in seq} | {spare}, rng)
        dyn("bad:control:%d" % k, tokens, lit_lens, dist_lens, valid=True, rle=seq, clens=clens)
        used_lit, used_dist = symbols_used(tokens)
        for what, lens, used in (("lit", lit_lens, used_lit), ("dist", dist_lens, used_dist)):
            def put(tag, new):
                a, b = (new, dist_lens) if what == "lit" else (lit_lens, new)
                writable = all(new[s] for s in used)
                dyn("bad:%s:%s:%d" % (tag, what, k), tokens if writable else [], a, b, rle=mode)
            new = list(lens)
            i = rng.choice([s for s in range(len(lens)) if lens[s] > 1])
            new[i] -= 1
            assert kraft(new) > 32768
            put("over", new)
            new = list(lens)
            i = rng.choice([s for s in range(len(lens)) if 0 < lens[s] < 15])
            new[i] += 1
            assert kraft(new) < 32768 and max(new) > 1
            put("longer", new)
            new = list(lens)
            i = rng.choice([s for s in range(len(lens)) if lens[s] and s not in used])
            new[i] = 0
            assert kraft(new) < 32768 and sorted(new)[-2] > 0
            put("dropped", new)
        new = list(clens)
        new[rng.choice([s for s in range(19) if clens[s] > 1])] -= 1
        dyn("bad:over:clen:%d" % k, tokens, lit_lens, dist_lens, rle=seq, clens=new)
        new = list(clens)
        new[rng.choice([s for s in range(19) if 0 < clens[s] < 7])] += 1
        dyn("bad:longer:clen:%d" % k, tokens, lit_lens, dist_lens, rle=seq, clens=new)
        new = list(clens)
        new[spare] = 0
        assert kraft(new) < 32768
        dyn("bad:dropped:clen:%d" % k, tokens, lit_lens, dist_lens, rle=seq, clens=new)
        # a repeat with nothing before it; repeats that run past the last length
        head = 3 + k % 4
        rest = cl_sequence(both[head:], mode)
        dyn("bad:first16:%d" % k, tokens, lit_lens, dist_lens, rle=[(16, head - 3)] + rest, clens=default_clens({16} | {s[0] for s in rest}, rng))
        for sym, extra, count in ((16, 3, 6), (17, 7, 10), (18, 127, 138)):
            cut = rng.randint(1, count - 1)                          # lengths left to say when the repeat of `count` comes
            front = cl_sequence(both[:-cut], "none" if sym == 16 else mode)
            if sym == 16 and front[-1][0] == 0:                      # (so that what is repeated is a length)
                front[-1] = (5,) + front[-1][1:]
            dyn("bad:past_end:%d:%d" % (sym, k), tokens, lit_lens, dist_lens, rle=front + [(sym, extra)],
                clens=default_clens({sym} | {s[0] for s in front}, rng))
        # no end-of-block code, in a set that is complete without it
        lits = sorted(s for s in symbols_used(tokens)[0] if s < 256)
        new = [0] * 257
        for s, l in zip(lits, complete_lengths(len(lits), rng, 15)):
            new[s] = l
        dyn("bad:eob0:%d" % k, [t for t in tokens if isinstance(t, int)], new + [0] * (len(lit_lens) - 257), dist_lens, rle=mode, eob=False)
        # more symbols than there are, the ones too many without a length
        for nl in (287, 288):
            dyn("bad:hlit%d:zero:%d" % (nl, k), tokens, lit_lens + [0] * (nl - len(lit_lens)), dist_lens, rle=mode)
        for nd in (31, 32):
            dyn("bad:hdist%d:zero:%d" % (nd, k), tokens, lit_lens, dist_lens + [0] * (nd - len(dist_lens)), rle=mode)
        # the member's size against isize, through a literal and through a match
        payload, plain, _ = member([("fixed", tokens)])
        if k < 6:
            for tag, more, delta in (("more:lit", [65], 0), ("more:match", [(3, 1)], 2), ("fewer:lit", [65], 2), ("fewer:match", [(3, 1)], 4)):
                p2, plain2, _ = member([("fixed", tokens + more)])
                L.bad("bad:%s:%d" % (tag, k), p2, len(plain) + delta, crc_of(plain2))
            L.bad("bad:trail:%d" % k, payload + bytes([rng.choice((0, 0, 255, 1))]), len(plain), crc_of(plain))
    # unused codes met in the data: the other bit of a single one-bit code, a length where there is no distance code at all
    for k in range(6):
        lits = [rng.choice(b"ACGT") for _ in range(10 + k)]
        lit_lens, _ = tables_for(lits + [(3, 1)], rng)
        for where in (0, 5):
            dist_lens = [0] * where + [1]
            dyn("bad:unused:dist_bit:%d:%d" % (where, k), lits + [("lsym", 257), ("bits", 1, 1), 65], lit_lens, dist_lens)
        dyn("bad:unused:no_dist:%d" % k, lits + [("lsym", 257), ("bits", 0, 1), 65], lit_lens, [0])
        dyn("bad:unused:no_dist30:%d" % k, lits + [("lsym", 257), ("bits", k, 3), 65], lit_lens, [0] * 30)
    one_bit = [0] * 256 + [1]
    dyn("bad:unused:lit_bit", [("bits", 1, 1)], one_bit, [0], eob=False)
    dyn("bad:unused:lit_bit_then_end", [("bits", 1, 1)], one_bit, [0], eob=True)
    # the code-length lengths of 16, 17, 18 and 0 alone: no length but zero can be said
    s = Stream()
    s.bits(1, 1); s.bits(2, 2); s.bits(0, 5); s.bits(0, 5); s.bits(0, 4)
    for l in (0, 0, 1, 1):
        s.bits(l, 3)
    s.code(1, 1); s.bits(127, 7); s.code(1, 1); s.bits(258 - 138 - 11, 7); s.bits(0, 8)
    L.bad("bad:hclen4:zeros", s.bytes(), 0)
    # symbols of the fixed code that stand for nothing
    for k in range(4):
        lits = [rng.getrandbits(8) for _ in range(k * 21 + 1)]
        for sym in (286, 287):
            for tail in ([], [("dsym", 0), 65]):
                p, plain, _ = member([("fixed", lits + [("lsym", sym)] + tail)])
                L.bad("bad:sym%d:%d:%d" % (sym, k, len(tail)), p, len(plain) + (0 if not tail else 4), crc_of(plain))
        for sym in (30, 31):
            for n in (3, 258):
                p, plain, _ = member([("fixed", lits + [("lsym", length_symbol(n)[0]), ("dsym", sym), ("bits", 0, 13), 65])])
                L.bad("bad:dsym%d:%d:%d" % (sym, k, n), p, len(lits) + n + 1, crc_of(plain))
    # a distance one beyond the bytes written, and one of exactly that many
    for pos in (1, 2, 3, 63, 64, 65, 100, 257):
        for n in (3, 64, 258):
            lits = [rng.getrandbits(8) for _ in range(pos)]
            L.blocks("bad:dist_pos:fixed:%d:%d" % (pos, n), [("fixed", lits + [(n, pos), 65])])
            L.blocks("bad:dist_pos:stored:%d:%d" % (pos, n), [("stored", bytes(lits)), ("fixed", [(n, pos), 65])])
            s = Stream()
            s.fixed_block(lits + [("lsym", length_symbol(n)[0]), ("bits", length_symbol(n)[2], length_symbol(n)[1])], True, eob=False)
            x = dist_symbol(pos + 1)
            s.code(x[0], 5); s.bits(x[2], x[1]); s.code(0, 7)
            L.bad("bad:dist_pos+1:fixed:%d:%d" % (pos, n), s.bytes(), pos + n)
            s = Stream()
            s.stored_block(bytes(lits), False)
            s.fixed_block([("lsym", length_symbol(n)[0]), ("bits", length_symbol(n)[2], length_symbol(n)[1])], True, eob=False)
            s.code(x[0], 5); s.bits(x[2], x[1]); s.code(0, 7)
            L.bad("bad:dist_pos+1:stored:%d:%d" % (pos, n), s.bytes(), pos + n)
    for k in range(6):
        s = Stream()
        for _ in range(k % 3):
            s.fixed_block(soup(rng, 50), False)
        s.bits(k % 2, 1); s.bits(3, 2); s.bits(0, 13)
        L.bad("bad:type3:%d" % k, s.bytes(), 50 * (k % 3))
    data = bytes(rng.getrandbits(8) for _ in range(300))
    for k, nlen in enumerate((300, 0, 0xffff, (300 ^ 0xffff) ^ 1, (300 ^ 0xffff) ^ 0x8000, (300 ^ 0xffff) + 1)):
        s = Stream()
        if k % 2:
            s.fixed_block([65] * 10, False)
        s.stored_block(data, True, nlen=nlen)
        L.bad("bad:nlen:%d" % k, s.bytes(), 300 + 10 * (k % 2), crc_of(b"A" * (10 * (k % 2)) + data))
    return L


def _crc_grid():
    """Stored members of 0..130 random bytes: the sizes at which the kernel's CRC has empty, clipped and whole 16-byte slices."""
    rng, L = random.Random(1007), _List()
    for n in range(131):
        L.blocks("crc:%d" % n, [("stored", bytes(rng.getrandbits(8) for _ in range(n)))])
    return L


_BUILDERS = dict(match_grid=_match_grid, chains=_chains, big_batches=_big_batches, blocks=_blocks, tables_ok=_tables_ok,
                 tables_bad=_tables_bad, crc_grid=_crc_grid)


@functools.lru_cache(maxsize=None)
def _built(name):
    """The list, every member judged by zlib's decoder: the class it was built for, and expand()'s bytes where accepted."""
    from tests.test_inflate_core_cpu import zlib_verdict
    L = _BUILDERS[name]()
    assert len(L.cases) <= 4000, (name, len(L.cases))
    for tag, payload, isize, crc in L.cases:
        verdict, out = zlib_verdict(payload, isize, crc)
        if tag in L.rejected:
            assert verdict == BAD_DEFLATE, (tag, verdict)
        else:
            assert (verdict, out) == (OK, L.plains[tag]), (tag, verdict)
    if name in ACCEPTED or name == "crc_grid":
        assert not L.rejected
    if name == "tables_bad":
        assert len(L.rejected) >= 200, len(L.rejected)
        for rule in BAD_RULES:
            assert any(t.startswith("bad:" + rule + ":") for t in L.rejected), rule
        for tag in L.plains:
            assert tag.split(":")[1] in BAD_VALID, tag
    return L


def cases(name):
    """[(tag, payload, isize, crc)] of a list, the same on every call"""
    return list(_built(name).cases)


def plains(name):
    """{tag: bytes} for the members of a list that zlib accepts"""
    return dict(_built(name).plains)


def profile(name):
    return dict(getattr(_built(name), "profile", {}))
