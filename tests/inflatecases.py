"""Designed deflate streams for the GPU inflate (csrc/bgzf_gpu.hip): a small deflate WRITER whose caller fixes the code lengths of
every symbol, the header's HLIT / HDIST / HCLEN, how the lengths are run-length coded and the symbol stream itself (and may ask for
streams no decoder should accept), the CASES built with it, and two short MODELS - of the lanes decoder's synchronisation and of
the rounds decoder's rounds - that only prove that a case reaches the edge it is named for.  Neither model is ever an expected
output: the reference of every byte is zlib (tests/test_cpu_inflate.py checks the cases against it without a GPU,
tests/test_gpu_inflate.py runs them through every form of the kernels).

Every size follows from the constants of the build (capi.bgzf_info()); TODAY is what they are in this tree.

A case: Case(name, family, streams, cls) with streams = [Stream]; a Stream is one BGZF block: the deflate bytes, the bytes the
writer meant (None for a stream no decoder should accept), the ISIZE its BGZF trailer declares and, where the edge needs it, the
`in_off & 3` of its first byte.  cls: "A" zlib accepts and the GPU must give the same bytes; "B" zlib rejects and so must the GPU;
"D" zlib accepts, the GPU has a stated limit and must report an error.  (Class "C" - zlib rejects, the kernel may not - is empty:
build_tables rejects the incomplete code sets zlib rejects, so those cases are in B.)"""
import struct
import zlib
from collections import namedtuple

TODAY = {"LIT_FAST": 11, "DIST_FAST": 9, "LANE_PART_BITS": 1024, "LANE_CHECK_BITS": 384, "LANE_FULL_WALKS": 8, "CHUNK_DW": 64, "RES_WIN": 16384,
         "RESOLVE_THREADS": 256, "BGZF_BATCH_BLOCKS": 16384, "BGZF_TOKENS_PER_BLOCK": 21846, "BGZF_MAX_DEFLATE_BLOCKS": 4096}
FORM_ROUNDS, FORM_SHARED = 1, 2
FORMS = {"lanes": 0, "rounds": FORM_ROUNDS, "lanes_shared": FORM_SHARED, "rounds_shared": FORM_ROUNDS | FORM_SHARED}
ALIGNS = (256, 1)
BGZF_MAX_STREAM = 65536 - 26  # deflate bytes that fit one BGZF block (BSIZE is 16 bits)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [x for x in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
EOB = 256


# ---- the writer -------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first bit writer (RFC 1951 3.1.1); Huffman codes go in most significant bit first"""

    def __init__(self):
        self.buf, self.acc, self.n, self.pos = bytearray(), 0, 0, 0

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        self.pos += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.bits(int(format(c & ((1 << n) - 1), "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.buf)


def canon_codes(lens):
    """canonical codes of a list of code lengths (RFC 1951 3.2.2); an over-subscribed set still gets codes (truncated to their length)"""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for L in range(1, 16):
        code = (code + cnt[L - 1]) << 1
        nxt[L] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else None)
        if l:
            nxt[l] += 1
    return out


def kraft(lens):
    """the code space a set of lengths takes, in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lengths(k):
    """k code lengths of a complete set, as even as possible (k >= 2)"""
    L = (k - 1).bit_length()
    short = (1 << L) - k
    return [L - 1] * short + [L] * (k - short)


def fill_complete(wanted):
    """wanted: {length: count}; adds one code for every set bit of the code space that is left: a complete set as {length: count}"""
    out = dict(wanted)
    left = 32768 - sum(c << (15 - l) for l, c in wanted.items())
    assert left >= 0
    for L in range(1, 16):
        if left & (1 << (15 - L)):
            out[L] = out.get(L, 0) + 1
    return out


def len_symbol(length):
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= length:
            return 257 + s, length - LEN_BASE[s]


def dist_symbol(dist):
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= dist:
            return s, dist - DIST_BASE[s]


def rle_plain(seq):
    return [(l,) for l in seq]


def rle_greedy(seq):
    """zero runs as 18 / 17, repeats as 16"""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        run = j - i
        if seq[i] == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r))
                run -= r
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [(0,)] * run
        else:
            out.append((seq[i],))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r))
                run -= r
            out += [(seq[i],)] * run
        i = j
    return out


def rle_expand(rle):
    out = []
    for it in rle:
        if it[0] < 16:
            out.append(it[0])
        elif it[0] == 16:
            out += [out[-1] if out else 0] * it[1]
        else:
            out += [0] * it[1]
    return out


Sym = namedtuple("Sym", "bit kind lsym lcode_len lbits dsym dcode_len dbits opos")  # bit: first bit; lbits / dbits: code + extra bits


class Deflate:
    """One raw deflate stream, block by block.  meta: one dict per block (type, hdr_bit, first_bit = the block's first code,
    ll / dl = the code lengths, syms = [Sym], eob_bit, end_bit, ntok); out: what the symbols written so far mean."""

    def __init__(self):
        self.w, self.out, self.meta, self.valid = BitWriter(), bytearray(), [], True

    def stored(self, data, final=False, len_field=None, nlen_field=None, cut=None):
        m = {"type": 0, "hdr_bit": self.w.pos}
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        ln = len(data) if len_field is None else len_field
        self.w.bits(ln, 16)
        self.w.bits((ln ^ 0xFFFF) if nlen_field is None else nlen_field, 16)
        m["first_bit"] = self.w.pos
        for b in (data if cut is None else data[:cut]):
            self.w.bits(b, 8)
        self.out += data
        m["end_bit"] = self.w.pos
        m["ntok"] = 0
        self.meta.append(m)
        return self

    def raw_bits(self, v, n):
        self.w.bits(v, n)
        return self

    def _symbols(self, m, syms, ll, dl):
        lc, dc = canon_codes(ll), canon_codes(dl)
        rec, ntok = [], 0
        for s in syms:
            bit, opos = self.w.pos, len(self.out)
            if isinstance(s, int):
                assert ll[s], "a symbol without a code"
                self.w.code(lc[s], ll[s])
                if s < 256:
                    self.out.append(s)
                if s == EOB:
                    m["eob_bit"] = bit
                rec.append(Sym(bit, "eob" if s == EOB else "lit" if s < 256 else "raw", s, ll[s], ll[s], None, 0, 0, opos))
                continue
            if s[0] == "x":  # explicit symbols and extra values: ("x", lsym, lextra, dsym or None, dextra)
                _, ls, lx, ds, dx = s
                length = LEN_BASE[ls - 257] + lx if 257 <= ls <= 285 else 0
                dist = DIST_BASE[ds] + dx if ds is not None and ds < 30 else 0
            else:  # (length, distance)
                length, dist = s
                ls, lx = len_symbol(length)
                ds, dx = dist_symbol(dist)
            assert ll[ls] and (ds is None or dl[ds]), "a symbol without a code"
            self.w.code(lc[ls], ll[ls])
            lxb = LEN_EXTRA[ls - 257] if 257 <= ls <= 285 else 0
            self.w.bits(lx, lxb)
            dbit = self.w.pos
            dxb = 0
            if ds is not None:
                self.w.code(dc[ds], dl[ds])
                dxb = DIST_EXTRA[ds] if ds < 30 else 0
                self.w.bits(dx, dxb)
            rec.append(Sym(bit, "match", ls, ll[ls], ll[ls] + lxb, ds, dl[ds] if ds is not None else 0, self.w.pos - dbit, opos))
            ntok += 1
            if dist and dist <= len(self.out):
                for _ in range(length):
                    self.out.append(self.out[-dist])
            else:
                self.valid = False
        m.update(syms=rec, ntok=ntok, end_bit=self.w.pos, ll=list(ll), dl=list(dl))
        self.meta.append(m)

    def fixed(self, syms, final=False):
        m = {"type": 1, "hdr_bit": self.w.pos}
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        m["first_bit"] = self.w.pos
        self._symbols(m, syms, FIXED_LL, FIXED_DL)
        return self

    def dynamic(self, syms, ll, dl, final=False, hlit=None, hdist=None, hclen=None, rle=None, cl_lens=None, btype=2):
        """ll / dl: code lengths by symbol (shorter lists are padded with zeros).  hlit / hdist: the numbers of lengths the header
        announces (default: up to the last used symbol).  rle: the code-length symbols as [(length,) | (16, rep) | (17, rep) | (18,
        rep)], default one symbol per length, "greedy" = rle_greedy of what the header announces; cl_lens: the 19 lengths of the code-length code, default a complete set over the symbols
        rle uses; hclen: how many of them are written."""
        ll, dl = list(ll) + [0] * (288 - len(ll)), list(dl) + [0] * (32 - len(dl))
        if hlit is None:
            hlit = max([257] + [i + 1 for i in range(288) if ll[i]])
        if hdist is None:
            hdist = max([1] + [i + 1 for i in range(32) if dl[i]])
        if rle is None or rle == "greedy":
            rle = (rle_greedy if rle else rle_plain)(ll[:hlit] + dl[:hdist])
        if cl_lens is None:
            used = sorted({it[0] for it in rle})
            if len(used) == 1:
                used.append(17 if used[0] != 17 else 18)
            cl_lens = [0] * 19
            for s, l in zip(used, complete_lengths(len(used))):
                cl_lens[s] = l
        if hclen is None:
            hclen = max(4, max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1)
        m = {"type": 2, "hdr_bit": self.w.pos, "hlit": hlit, "hdist": hdist, "hclen": hclen, "rle": rle, "cl_lens": cl_lens}
        self.w.bits(int(final), 1)
        self.w.bits(btype, 2)
        self.w.bits(hlit - 257, 5)
        self.w.bits(hdist - 1, 5)
        self.w.bits(hclen - 4, 4)
        for i in range(hclen):
            self.w.bits(cl_lens[CL_ORDER[i]], 3)
        cc = canon_codes(cl_lens)
        for it in rle:
            self.w.code(cc[it[0]] or 0, cl_lens[it[0]])
            if it[0] == 16:
                self.w.bits(it[1] - 3, 2)
            elif it[0] == 17:
                self.w.bits(it[1] - 3, 3)
            elif it[0] == 18:
                self.w.bits(it[1] - 11, 7)
        m["first_bit"] = self.w.pos
        self._symbols(m, syms, ll, dl)
        return self

    def bytes(self):
        return self.w.done()


class Stream:
    def __init__(self, d, intended="auto", isize=None, in_align=None, cut=None):
        self.data = d.bytes() if cut is None else d.bytes()[:cut]
        self.meta = d.meta
        self.intended = (bytes(d.out) if d.valid else None) if intended == "auto" else intended
        self.isize = isize if isize is not None else (len(self.intended) if self.intended is not None else max(1, len(d.out)))
        self.in_align = in_align
        assert len(self.data) <= BGZF_MAX_STREAM and self.isize <= 65536, (len(self.data), self.isize)


Case = namedtuple("Case", "name family streams cls")


def bgzf_image(streams, start=0):
    """the streams as BGZF blocks back to back, without the empty end-of-file block: (bytes, [in_off of every stream]).  A stream that
    asks for an `in_off & 3` gets a second extra subfield of the size that gives it."""
    out, offs, off = [], [], start
    for s in streams:
        pad = None
        if s.in_align is not None:
            for p in range(4):
                if (off + 12 + 6 + 4 + p) & 3 == s.in_align:
                    pad = p
        extra = b"BC\x02\0" + struct.pack("<H", len(s.data) + 25 + (0 if pad is None else 4 + pad))
        if pad is not None:
            extra += b"ZZ" + struct.pack("<H", pad) + bytes(pad)
        blk = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(extra)) + extra + s.data + struct.pack("<II", zlib.crc32(s.intended or b""), s.isize)
        assert len(blk) <= 65536
        offs.append(off + 12 + len(extra))
        out.append(blk)
        off += len(blk)
    return b"".join(out), offs


# ---- the models (proofs that a case reaches its edge; never an expected output) ---------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.d = data + bytes(8)

    def peek(self, pos):
        return int.from_bytes(self.d[pos >> 3:(pos >> 3) + 6], "little") >> (pos & 7)


def _decoder(lens):
    return {(l, c): s for s, (l, c) in enumerate(zip(lens, canon_codes(lens))) if l}


def _decode(bits, pos, tab):
    w, code = bits.peek(pos), 0
    for L in range(1, 16):
        code = (code << 1) | ((w >> (L - 1)) & 1)
        s = tab.get((L, code))
        if s is not None:
            return s, L
    return None, 0


def _lane_walk(bits, lt, dt, pos, until, end_bit):
    """lane_segment: one lane walks from `pos` until its next literal/length code lies at or beyond `until`; (pos, stop) with stop
    None / "eob" / "bad" and pos = behind the end-of-block code for "eob" """
    while pos < until:
        s, L = _decode(bits, pos, lt)
        if s is None or s > 285:
            return pos, "bad"
        pos += L
        if s == EOB:
            return pos, ("bad" if pos > end_bit else "eob")
        if s > 256:
            pos += LEN_EXTRA[s - 257]
            if pos > end_bit:
                return pos, "bad"
            d, L = _decode(bits, pos, dt)
            if d is None or d > 29:
                return pos, "bad"
            pos += L + DIST_EXTRA[d]
        if pos > end_bit:
            return pos, "bad"
    return pos, None


def sync_model(stream, block, info=TODAY):
    """lanes_block on Huffman block `block` of a stream: one dict per window - passes, long (passes that needed a walk beyond the
    checkpoint, the window's first included) and rounds (True: the window, and with it the rest of the block, is left to the
    rounds decoder)."""
    PART, CHECK, FULL = info["LANE_PART_BITS"], info["LANE_CHECK_BITS"], info["LANE_FULL_WALKS"]
    m = stream.meta[block]
    bits, lt, dt, end_bit = _Bits(stream.data), _decoder(m["ll"]), _decoder(m["dl"]), 8 * len(stream.data)
    cur, wins, NONE = m["first_bit"], [], None
    while True:
        s = [cur + i * PART for i in range(64)]
        limit = [min(x + PART, end_bit) for x in s]
        check = [min(x + CHECK, l) for x, l in zip(s, limit)]
        ref_entry, cp_pos, ref_exit = [NONE] * 64, [NONE] * 64, [NONE] * 64
        entry, exitv, need = [x if x < end_bit else NONE for x in s], [NONE] * 64, [True] * 64
        passes = long = 0
        for _ in range(66):
            passes += 1
            walked, any_long = [], False
            for i in range(64):
                if not (need[i] and entry[i] is not NONE and entry[i] < limit[i] and entry[i] != ref_entry[i]):
                    continue
                pos, stop = _lane_walk(bits, lt, dt, entry[i], check[i], end_bit)
                if not stop and cp_pos[i] is not NONE and pos == cp_pos[i]:
                    continue  # joined the reference walk at its checkpoint
                walked.append((i, pos, stop))
                any_long |= not stop and pos < limit[i]
            if any_long:
                long += 1
                if long > FULL:
                    wins.append({"passes": passes, "long": long, "rounds": True})
                    return wins
            for i, pos, stop in walked:
                ref_entry[i], cp_pos[i] = entry[i], (NONE if stop else pos)
                if not stop and pos < limit[i]:
                    pos, stop = _lane_walk(bits, lt, dt, pos, limit[i], end_bit)
                ref_exit[i] = (pos, stop)
            for i in range(64):
                if need[i]:
                    exitv[i] = (entry[i], None) if entry[i] is NONE or entry[i] >= limit[i] else ref_exit[i]
            new = []
            for i in range(64):
                ne = cur if i == 0 else (NONE if exitv[i - 1][1] else exitv[i - 1][0])
                if ne is not NONE and ne >= end_bit:
                    ne = NONE
                new.append(ne)
            need = [a != b for a, b in zip(new, entry)]
            entry = new
            if not any(need):
                break
        wins.append({"passes": passes, "long": long, "rounds": False})
        stops = [i for i in range(64) if entry[i] is not NONE and exitv[i][1]]
        if stops:
            assert exitv[stops[0]][1] == "eob", "the model met a malformed block"
            return wins
        assert all(e is not NONE for e in entry), "the stream ends inside the window"
        cur = exitv[63][0]


def rounds_model(stream, block, info=TODAY):
    """the rounds decoder on Huffman block `block`, from the symbols the writer recorded: [(Sym, where)] with where = "head" (first
    symbol of a round), "mid" (later in a round; a literal/length code longer than the direct table is then decoded by the fix-up
    in either place) or "scalar" (a match whose distance code is longer than the direct table: the chain of its round stops in front
    of it, it is the head of the next round, does not decode there and goes to the scalar path with walk_code)"""
    DF = info["DIST_FAST"]
    out, head, rstart = [], True, 0
    for s in stream.meta[block]["syms"]:
        if head:
            rstart = s.bit
        if s.kind == "match" and s.dcode_len > DF:
            out.append((s, "scalar"))
            head = True
            continue
        out.append((s, "head" if head else "mid"))
        head = s.bit + s.lbits + s.dbits - rstart >= 64  # the chain ends with the symbol that ends at or beyond bit 64
    return out


# ---- helpers of the cases ---------------------------------------------------------------------------------------------------------
def lcg_bytes(n, seed, lo=0, hi=256):
    out, x = bytearray(), seed * 2654435761 % (1 << 32) or 1
    for _ in range(n):
        x = (x * 1664525 + 1013904223) % (1 << 32)
        out.append(lo + (x >> 16) % (hi - lo))
    return bytes(out)


def lcg_pick(items, n, seed):
    return [items[b % len(items)] for b in lcg_bytes(n, seed)]


def fill_matches(n, dist, length=258):
    """matches of `length` (the last one shorter, never below 3) that give n bytes"""
    out = []
    while n:
        k = min(n, length)
        if 0 < n - k < 3:
            k -= 3 - (n - k)
        out.append((k, dist))
        n -= k
    return out


def fixed_literals_to_bit(target, seed):
    """literals of the fixed code that take exactly `target` bits: 8-bit ones (< 144) and as many 9-bit ones as target % 8 asks for"""
    nine = target % 8
    eight = (target - 9 * nine) // 8
    lits = list(lcg_bytes(eight, seed, 0, 144))
    step = max(1, eight // (nine + 1))
    for k in range(nine):
        lits.insert((k + 1) * step, 144 + k)
    return lits


def table(assign, n):
    lens = [0] * n
    for s, l in assign.items():
        lens[s] = l
    return lens


# lit/len table with codes of exactly LIT_FAST, LIT_FAST + 1 and 15 bits on a literal (the first code of the length) and on a length
# symbol (the last); short codes for the text; EOB short (variant 0) or the all-ones 15-bit code (variant 1, with 285 zero)
def long_tables(info, variant):
    LF, DF = info["LIT_FAST"], info["DIST_FAST"]
    ll = {}
    text = [65, 67, 71, 84, 78, 10, 9, 48, 49, 50, 51, 52]
    wanted = {LF: 4, LF + 1: 3, 15: 3 if variant == 0 else 4}
    counts = fill_complete(wanted)
    pool = {LF: [200, 201, 257, 265], LF + 1: [202, 203, 270], 15: [204, 205, 285] if variant == 0 else [204, 205, 255, EOB]}
    rest = iter(text + [258, 259, 260, 266, 274, 280, 284, 97, 98, 99, 100, 101, 102])
    if variant == 0:
        ll[EOB] = min(l for l in counts if counts[l] > wanted.get(l, 0))
    for L in sorted(counts):
        free = counts[L] - (len(pool[L]) if L in pool else 0) - (1 if variant == 0 and ll.get(EOB) == L else 0)
        for s in pool.get(L, []):
            ll[s] = L
        for _ in range(free):
            ll[next(rest)] = L
    dcounts = fill_complete({DF: 2, DF + 1: 2, 15: 2})
    dpool = {DF: [2, 20], DF + 1: [3, 21], 15: [4, 29]}
    drest = iter([0, 1, 5, 6, 8, 10, 12, 14, 16, 18, 22, 24, 26, 28, 7, 9, 11, 13])
    dl = {}
    for L in sorted(dcounts):
        for s in dpool.get(L, []):
            dl[s] = L
        for _ in range(dcounts[L] - len(dpool.get(L, []))):
            dl[next(drest)] = L
    return table(ll, 286), table(dl, 30)


def build_cases(info=TODAY):
    LF, DF, PART, CHECK = info["LIT_FAST"], info["DIST_FAST"], info["LANE_PART_BITS"], info["LANE_CHECK_BITS"]
    FULL, CHUNK, RW, MAXB = info["LANE_FULL_WALKS"], info["CHUNK_DW"], info["RES_WIN"], info["BGZF_MAX_DEFLATE_BLOCKS"]
    cases = []

    def add(name, family, streams, cls="A"):
        cases.append(Case(name, family, streams if isinstance(streams, list) else [streams], cls))

    # ---- code lengths: every long code, first and last of its length, as literal / length / distance, mixed so that rounds meet
    # them at their head and later, and the lanes under a checkpoint (tests/test_cpu_inflate.py proves where they fall)
    for variant in (0, 1):
        ll, dl = long_tables(info, variant)
        lits = [s for s in range(256) if ll[s]]
        lens_ = [s for s in range(257, 286) if ll[s]]
        dists = [s for s in range(30) if dl[s]]
        d = Deflate().stored(lcg_bytes(40000 if variant == 0 else 33000, 7 + variant))
        syms, opos = [], len(d.out)
        picks = lcg_bytes(5200, 11 + variant)
        for i, b in enumerate(picks):
            if b % 3:
                syms.append(lits[(b // 3) % len(lits)])
                opos += 1
            else:
                ls = lens_[(b // 3) % len(lens_)]
                cand = [x for x in dists if DIST_BASE[x] + (1 << DIST_EXTRA[x]) - 1 <= opos]
                ds = cand[picks[(i * 7 + 3) % len(picks)] % len(cand)]
                lx, dx = (b >> 2) % (1 << LEN_EXTRA[ls - 257]), (1 << DIST_EXTRA[ds]) - 1 if b & 64 else 0
                if opos + LEN_BASE[ls - 257] + lx > 60000:
                    continue
                syms.append(("x", ls, lx, ds, dx))
                opos += LEN_BASE[ls - 257] + lx
        d.dynamic(syms + [EOB], ll, dl, final=True, rle="greedy")
        add("long_codes_eob_%s" % ("short" if variant == 0 else "all_ones_15"), "codes", Stream(d))

    # ---- every length code and every distance code at its smallest and largest extra value; distance 32768 at position 32768
    def extremes(d, first_match_pos):
        assert len(d.out) == first_match_pos
        syms = [("x", 285, 0, 29, (1 << 13) - 1)]  # distance 32768 at output position 32768
        for ls in range(257, 286):
            for lx in {0, (1 << LEN_EXTRA[ls - 257]) - 1}:
                syms.append(("x", ls, lx, (ls * 7) % 30, 0))
        for ds in range(30):
            for dx in {0, (1 << DIST_EXTRA[ds]) - 1}:
                syms += [ds * 8 + 1, ("x", 257 + ds % 28, 0, ds, dx)]
        return syms

    d = Deflate().stored(lcg_bytes(32768, 3))
    d.fixed(extremes(d, 32768) + [EOB], final=True)
    add("extras_fixed_dist32768_at_32768_into_stored", "extras", Stream(d))
    d = Deflate().stored(lcg_bytes(32768, 4))
    d.dynamic(extremes(d, 32768) + [EOB], complete_lengths(286), complete_lengths(30), final=True, rle="greedy")
    add("extras_dynamic_hlit286_hdist30", "extras", Stream(d))
    d = Deflate().stored(lcg_bytes(300, 5)).fixed([1, 2, ("x", 284, 31, 0, 0), 3, EOB], final=True)
    ok = True
    try:
        zlib.decompress(d.bytes(), -15)
    except zlib.error:
        ok = False
    add("extras_284_with_extra_31", "extras", Stream(d, intended="auto" if ok else None), "A" if ok else "B")

    # ---- headers
    abc = {97: 1, 98: 2, EOB: 2}
    text = lcg_pick([97, 97, 98], 300, 21)
    d = Deflate().dynamic(text + [EOB], table(abc, 257), [0], final=True, hlit=257, hdist=1)
    add("hlit257_hdist1_one_zero_distance_length", "headers", Stream(d))
    ll8 = [8] * 255 + [0, 8]
    d = Deflate().dynamic(list(lcg_bytes(500, 22, 0, 255)) + [EOB], ll8, [0], final=True, rle=[(8,), (16, 6)] * 36 + [(8,)] * 3 + [(0,), (8,), (0,)],
                          cl_lens=table({8: 1, 0: 2, 16: 2}, 19))
    assert d.meta[0]["hclen"] == 5 and rle_expand(d.meta[0]["rle"]) == ll8 + [0]
    add("hclen5_the_smallest_that_can_name_a_code", "headers", Stream(d))
    full = complete_lengths(286)
    d = Deflate().stored(b"0123456789").dynamic([48, 49, (5, 10), 200, EOB], full, complete_lengths(30), final=True, cl_lens=[4] * 16 + [0] * 3, hclen=19)
    add("hclen19_every_code_length_code_4_bits", "headers", Stream(d))
    d = Deflate().stored(b"ab").dynamic(text[:50] + [(4, 2), (3, 1), (5, 4), (3, 3), EOB], table({97: 1, 98: 3, 257: 3, 258: 3, 259: 4, EOB: 4}, 260), [2, 2, 2, 2], final=True)
    add("plain_header_small_tables", "headers", Stream(d))
    # code 16 runs from the literal/length lengths into the distance lengths: ... EOB 2 | 2 2 2 2 as (2,) (16, 4)
    seq = table(abc, 257)
    d = Deflate().stored(b"ab").dynamic(text[:40] + [EOB], seq, [2, 2, 2, 2], final=True, hlit=257, hdist=4, rle=rle_greedy(seq[:256]) + [(2,), (16, 4)])
    assert rle_expand(d.meta[1]["rle"]) == seq + [2, 2, 2, 2]
    add("code16_repeats_across_the_literal_distance_boundary", "headers", Stream(d))
    seq = table({1: 2, 255: 2, EOB: 1}, 257)
    d = Deflate().dynamic(lcg_pick([1, 255], 100, 23) + [EOB], seq, [0], final=True, rle=[(0,), (2,), (18, 138), (18, 115), (2,), (1,), (0,)])
    assert rle_expand(d.meta[0]["rle"]) == seq + [0]
    add("code18_with_138", "headers", Stream(d))
    d = Deflate().dynamic([97, (200, 1), 98, (3, 1), EOB], table({**abc, 98: 3, 257: 4, 269: 5, 283: 5}, 284), [1], final=True)
    add("lone_1_bit_distance_code", "headers", Stream(d))
    d = Deflate().stored(b"xyz").dynamic([EOB], table({EOB: 1}, 257), [0], final=True)
    add("literal_length_set_of_a_1_bit_end_of_block_alone", "headers", Stream(d))
    d = Deflate().dynamic(text[:100] + [EOB], table(abc, 257), [0]).fixed(list(lcg_bytes(100, 24)) + [(50, 120), EOB]).dynamic(text[:60] + [(5, 2), EOB], table({**abc, 98: 3, 259: 3}, 260), [1, 1],
                                                                                                                       final=True)
    add("fixed_directly_after_dynamic_then_dynamic", "headers", Stream(d))

    # ---- stored blocks
    d = Deflate().stored(b"").stored(b"q").stored(b"").fixed([1, 2, 3, (3, 4), EOB], final=True)
    add("stored_len_0_and_1", "stored", Stream(d))
    big = BGZF_MAX_STREAM - 5
    add("stored_len_%d_the_longest_a_bgzf_block_holds" % big, "stored", Stream(Deflate().stored(lcg_bytes(big, 31), final=True)))
    for nine, endbit in ((3, 5), (4, 6)):
        d = Deflate().fixed([5, 6] + [200 + k for k in range(nine)] + [EOB])
        assert d.w.pos % 8 == endbit
        d.stored(lcg_bytes(77, 32)).fixed([(30, 50), EOB], final=True)
        add("stored_after_huffman_block_ending_at_bit_%d%s" % (endbit, "_no_padding" if endbit == 5 else ""), "stored", Stream(d))
    for al in range(4):
        for ahead in (CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK):
            if al and ahead != CHUNK:
                continue
            n = 4 * ahead - 5 - al
            d = Deflate().stored(lcg_bytes(n, 33 + ahead))
            assert (al * 8 + d.w.pos) >> 5 == ahead
            d.fixed([7, (100, n), 8, (20, 3), EOB], final=True)
            add("stored_then_header_%d_dwords_ahead_in_off_%d" % (ahead, al), "stored", Stream(d, in_align=al))

    # ---- sizes
    for isize in (65533, 65534, 65535, 65536, RW - 3, RW - 2, RW - 1, RW + 1, RW + 2, RW + 3, 2 * RW + 1):
        pre = 5000 + isize % 7
        d = Deflate().stored(lcg_bytes(pre, isize)).fixed(fill_matches(isize - pre, pre - 1) + [EOB], final=True)
        add("isize_%d" % isize, "sizes", Stream(d))
    d = Deflate().fixed([90] + [(3, 1)] * 21845 + [EOB], final=True)
    add("one_literal_and_21845_matches_of_3", "sizes", Stream(d))
    d = Deflate()
    for k in range(MAXB):
        d.fixed([k % 251, EOB], final=k == MAXB - 1)
    add("%d_deflate_blocks" % MAXB, "sizes", Stream(d))
    d = Deflate()
    for k in range(MAXB + 1):
        d.fixed([k % 251, EOB], final=k == MAXB)
    add("%d_deflate_blocks" % (MAXB + 1), "limits", Stream(d), "D")

    # ---- lanes geometry (fixed code)
    W = 64 * PART
    for eob_at in (W - 1, W, W + 1):
        d = Deflate().fixed(fixed_literals_to_bit(eob_at, 41) + [EOB], final=True)
        add("end_of_block_code_at_bit_%d" % eob_at, "geometry", Stream(d))
    add("stream_ends_inside_lane_0", "geometry", Stream(Deflate().fixed([1, 2, 3, (5, 2), EOB], final=True)))
    for delta in (-1, 0, 1):
        lits = fixed_literals_to_bit(3 * PART - 7 + delta, 42)  # a 7-bit length code (257 .. 264, no extra bits) behind them
        d = Deflate().fixed(lits + [(8, 100), 9, 10] + list(lcg_bytes(300, 43)) + [EOB], final=True)
        add("length_code_ends_%+d_bits_from_a_part_boundary" % delta, "geometry", Stream(d))
    d = Deflate().fixed(list(lcg_bytes(9000, 44)) + fill_matches(3000, 777) + list(lcg_bytes(8500, 45)) + [EOB], final=True)
    add("three_windows", "geometry", Stream(d))

    # ---- synchronisation
    # 255 literals and the end of block at 8 bits: a part is a multiple of 8 bits long, so every lane starts on a code and the very
    # first pass is the last (random bytes do not make a block that never synchronises; the runs of one bits below do)
    d = Deflate().dynamic(list(lcg_bytes(3000, 51, 0, 255)) + [EOB], ll8, [0], final=True, rle="greedy")
    add("every_code_8_bits_every_part_starts_on_a_code", "sync", Stream(d))
    # literals 0 .. 127 have the 8-bit codes 1xxxxxxx, so a run of literal 127 is a run of one bits: a walk from a wrong bit stays wrong
    st = {**{s: 8 for s in range(128)}, 200: 3, 201: 3, 202: 4, 203: 4, 204: 5, 205: 5, 206: 6, 207: 6, 208: 6, EOB: 6}
    stl = table(st, 257)
    words = [200, 201, 202, 203, 204, 205, 206, 207, 208, 3, 77]

    lead = {}

    def stretch_case(p, where):
        if where not in lead:  # the run starts in window `where`, a few parts in and 3 bits off the part grid
            syms, k, want = [], 0, where * 64 * PART + 3 * PART
            while True:
                d0 = Deflate().dynamic(syms, stl, [0], rle="greedy")
                at = d0.w.pos - d0.meta[0]["first_bit"]
                if at >= want and at % 8 == 3:
                    break
                syms += lcg_pick(words, max(8, (want - at) // 5), 53 + k) if at < want else [204]
                k += 1
            lead[where] = syms
        body = lead[where] + [127] * (p * PART // 8) + lcg_pick(words, 3000, 54) + [EOB]
        return Stream(Deflate().dynamic(body, stl, [0], final=True, rle="greedy"))

    for where in (0, 1):
        for p in range(FULL - 2, FULL + 2):
            s = stretch_case(p, where)
            wins = sync_model(s, 0, info)
            add("unsynchronised_stretch_of_%d_parts_in_window_%d_long_passes_%s" % (p, where, "_".join(str(w["long"]) for w in wins)) + ("_to_the_rounds" if wins[-1]["rounds"] else ""),
                "sync", s)
    # the same with codes above both direct tables inside the stretch: length symbol 264 and distance symbol 5 have the all-ones 15-bit
    # codes, (10, 8) is 15 + 15 + 1 one bits
    cl = {65 + k: k + 1 for k in range(13)}
    cl.update({EOB: 14, 263: 15, 264: 15})
    cd = {6 + k: k + 1 for k in range(14)}
    cd.update({4: 15, 5: 15})
    cll, cdl = table(cl, 265), table(cd, 20)
    assert kraft(cll) == kraft(cdl) == 32768
    ctext = [65, 65, 65, 66, 66, 67, 68, 69]
    for where in (0, 1):
        lead = lcg_pick(ctext, 40000, 55) if where else []
        body = lead + lcg_pick(ctext, 500, 56) + [70] + [(10, 8)] * ((FULL + 4) * PART // 31) + lcg_pick(ctext, 2000, 57) + [EOB]
        s = Stream(Deflate().dynamic(body, cll, cdl, final=True, rle="greedy"))
        wins = sync_model(s, 0, info)
        add("unsynchronised_stretch_of_15_bit_length_and_distance_codes_in_window_%d_long_passes_%s" % (where, "_".join(str(w["long"]) for w in wins))
            + ("_to_the_rounds" if wins[-1]["rounds"] else ""), "sync", s)

    # ---- resolve
    for back in (1, 257, 258):
        at = RW - back
        d = Deflate().stored(lcg_bytes(at, 61 + back)).fixed([(258, 300), 1, 2, 3, (258, 100), EOB], final=True)
        add("match_of_258_starting_%d_before_the_resolve_window_edge" % back, "resolve", Stream(d))
    d = Deflate().stored(lcg_bytes(RW + 100, 64)).fixed([(258, RW), (100, RW + 50), 5, (30, RW + 389), EOB], final=True)
    add("match_source_wholly_in_an_earlier_window", "resolve", Stream(d))
    d = Deflate().fixed([33] + fill_matches(65535, 1) + [EOB], final=True)
    add("distance_1_run_across_four_windows", "resolve", Stream(d))
    d = Deflate().fixed([1, 2, 3] + [(3, 3)] * 7000 + [4, 5, 6, 7, 8] + [(258, 5)] * 100 + [EOB], final=True)
    add("chain_of_matches_each_copying_the_one_before", "resolve", Stream(d))
    d = Deflate().fixed(list(lcg_bytes(50, 65)) + fill_matches(RW - 50 - 10, 50) + [EOB]).stored(lcg_bytes(RW + 20, 66)).fixed(fill_matches(3000, 2 * RW) + [EOB], final=True)
    add("resolve_window_with_no_token_starting_in_it", "resolve", Stream(d))

    # ---- class B: zlib rejects on structure
    def bad(name, d, **kw):
        add(name, "invalid", Stream(d, intended=None, **kw), "B")

    pre = b"0123456789"
    bad("block_type_3", Deflate().stored(pre).raw_bits(0b111, 3).raw_bits(0, 29))
    bad("nlen_mismatch", Deflate().stored(pre, final=True, nlen_field=0x1234))
    bad("stored_len_beyond_the_stream", Deflate().stored(pre * 10, final=True, cut=50))
    for f in (30, 31):
        bad("hlit_field_%d" % f, Deflate().stored(pre).dynamic([1, EOB], complete_lengths(257 + f), [1, 1], final=True, hlit=257 + f))
    for f in (30, 31):
        bad("hdist_field_%d" % f, Deflate().stored(pre).dynamic([1, EOB], complete_lengths(257), complete_lengths(f + 1), final=True, hdist=f + 1))
    seq = table(abc, 257) + [0]
    bad("code16_as_the_first_length", Deflate().stored(pre).dynamic([97, EOB], table(abc, 257), [0], final=True, rle=[(16, 3)] + rle_greedy(seq[3:])))
    bad("repeat_overruns_hlit_plus_hdist", Deflate().stored(pre).dynamic([97, EOB], table(abc, 257), [0], final=True, rle=rle_greedy(seq[:256]) + [(2,), (17, 3)]))
    bad("hclen4_can_name_no_code", Deflate().stored(pre).dynamic([], [0] * 257, [0], final=True, rle=[(18, 138), (18, 120)], cl_lens=table({18: 1, 0: 1}, 19), hclen=4))
    bad("no_end_of_block_code", Deflate().stored(pre).dynamic([97, 98, 97], table({97: 1, 98: 1}, 257), [0], final=True))
    bad("oversubscribed_code_length_code", Deflate().stored(pre).dynamic([97, EOB], table(abc, 257), [0], final=True, cl_lens=table({0: 1, 1: 1, 2: 1, 18: 2}, 19)))
    bad("oversubscribed_literal_length_set", Deflate().stored(pre).dynamic([97, EOB], table({97: 1, 98: 1, EOB: 1}, 257), [0], final=True))
    bad("oversubscribed_distance_set", Deflate().stored(pre).dynamic([97, EOB], table(abc, 257), [1, 1, 1], final=True))
    for s in (286, 287):
        bad("fixed_symbol_%d" % s, Deflate().stored(pre).fixed([1, 2, s, 3, EOB], final=True))
    for s in (30, 31):
        bad("fixed_distance_%d" % s, Deflate().stored(pre).fixed([1, 2, ("x", 257, 0, s, 0), 3, EOB], final=True))
    bad("distance_beyond_the_start_first_match", Deflate().stored(pre).fixed([(3, 11), 1, EOB], final=True))
    bad("distance_beyond_the_start_mid_block", Deflate().stored(pre).fixed(list(lcg_bytes(2000, 71)) + [(5, 100), (3, 2016), 1, EOB], final=True))
    ll, dl = long_tables(info, 0)
    lit0 = [x for x in range(256) if ll[x]][:6]
    assert dl[3] == DF + 1 and dl[21] == DF + 1 and ll[257]
    bad("distance_beyond_the_start_first_match_long_distance_code", Deflate().stored(b"abc").dynamic([(3, 4), lit0[0], EOB], ll, dl, final=True, rle="greedy"))
    bad("distance_beyond_the_start_mid_block_long_distance_code",
        Deflate().stored(pre).dynamic(lcg_pick(lit0, 1590, 72) + [(3, 1601), lit0[0], EOB], ll, dl, final=True, rle="greedy"))
    d = Deflate().stored(pre).fixed(list(lcg_bytes(300, 73)) + [(40, 30)] * 20 + [EOB], final=True)
    bad("stream_ends_before_the_end_of_block", d, cut=len(d.bytes()) - 40, isize=10 + 300 + 800)
    good = Deflate().stored(pre).fixed(list(lcg_bytes(300, 74)) + [(40, 30)] * 20 + [EOB], final=True)
    for delta in (1, -1):
        add("output_one_byte_%s_than_isize" % ("fewer" if delta == 1 else "more"), "invalid", Stream(good, isize=len(good.out) + delta), "B")
    bad("length_code_without_distance_codes", Deflate().stored(pre).dynamic([97, 98, ("x", 257, 0, None, 0), 97, 97, 97, 97, EOB], table({97: 1, 98: 2, 257: 3, EOB: 3}, 258), [0], final=True))
    # what zlib rejects as an incomplete set although the stream uses assigned codes only (once class C: build_tables now rejects them)
    bad("incomplete_literal_length_set", Deflate().stored(pre).dynamic([97, 98, 97, EOB], table({97: 1, 98: 2, EOB: 3}, 257), [0], final=True))
    bad("incomplete_distance_set", Deflate().stored(pre).dynamic([97, 98, (4, 2), (3, 1), EOB], table({97: 1, 98: 2, 257: 4, 258: 4, EOB: 3}, 259), [2, 2, 2], final=True))
    bad("incomplete_code_length_code", Deflate().stored(pre).dynamic([97, EOB], table(abc, 257), [0], final=True, cl_lens=table({0: 1, 1: 2, 2: 3, 18: 4}, 19)))
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    return cases


FAMILIES = ("codes", "extras", "headers", "stored", "sizes", "geometry", "sync", "resolve")
_CACHE = {}


def cases(info=TODAY):
    key = tuple(sorted(info.items()))
    if key not in _CACHE:
        _CACHE[key] = build_cases(info)
    return _CACHE[key]


_ZREF = {}


def zlib_reference(stream):
    """what zlib makes of a stream: its bytes, or None where it raises; computed once per stream"""
    if id(stream) not in _ZREF:
        try:
            _ZREF[id(stream)] = (stream, zlib.decompress(stream.data, -15))
        except zlib.error as e:
            _ZREF[id(stream)] = (stream, None, str(e))
    return _ZREF[id(stream)][1]


def zlib_error(stream):
    zlib_reference(stream)
    r = _ZREF[id(stream)]
    return r[2] if len(r) > 2 else None


def bgzf_scratch_bytes(nblk, info=TODAY):
    """what launch_bgzf_inflate asks for (csrc/bgzf_gpu.h)"""
    return min(nblk, info["BGZF_BATCH_BLOCKS"]) * (info["BGZF_TOKENS_PER_BLOCK"] * 8 + 4) + 64


def batch_image(info=TODAY):
    """BGZF_BATCH_BLOCKS + 1 blocks: one byte each but for three designed ones at the last index of the first launch pair, the
    first of the second and the one before; (image, [expected bytes per block])"""
    n = info["BGZF_BATCH_BLOCKS"] + 1
    by = {c.name: c for c in cases(info)}
    designed = {n - 3: by["chain_of_matches_each_copying_the_one_before"].streams[0], n - 2: by["one_literal_and_21845_matches_of_3"].streams[0],
                n - 1: by["three_windows"].streams[0]}
    streams, small = [], {}
    for i in range(n):
        if i in designed:
            streams.append(designed[i])
        else:
            b = i % 251
            if b not in small:
                small[b] = Stream(Deflate().fixed([b, EOB], final=True))
            streams.append(small[b])
    img, _ = bgzf_image(streams)
    return img, streams
