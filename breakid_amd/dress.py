"""The "dresser": writes the records of a synth.Dataset the way an aligner leaves them - packed bases, qualities and typed aux
fields around SA / OC - for the feed tests (tests/dresscases.py), tools/make_golden.py and tools/gpu_feedfuzz.py.  Tooling like
synth / bamio, not the product's path.  The fields the path reads stay as they are, so the expected table of a dressed file is
still ds.to_soa(), bit for bit; everything else is seeded, real-shaped and hostile.  LAYOUTS are hand-written aux areas, one
per read, each with its name and the blob it must decode to."""
import random
import struct
from collections import namedtuple

from . import bamio, synth

L_SEQS = (0, 1, 36, 101, 150, 251)                 # odd and even: the offset (l_seq + 1) / 2 + l_seq
DECOY_SA = b"SAZchr2,5,+,60S40M,60,0;"             # values that spell fields (each is followed by a NUL where it lies)
DECOY_OC = b"OCZ10M"
DECOY_BYTES = DECOY_SA + b"\0" + DECOY_OC + b"\0"
SCALAR_KINDS = list("AcCsSiIfdZH")
ARRAY_KINDS = ["B" + s for s in bamio.AUX_ARRAY_SUBTYPES]
KINDS = SCALAR_KINDS + ARRAY_KINDS
BIG = 3001                                         # elements of a long array: more than a quarter of a BGZF block for 4-byte types
_INT_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}
_SAZC = struct.unpack("<I", b"SAZc")[0]
_SEED = 20240611


def kind_of(item):
    """'A' .. 'H', 'Bc' .. 'Bf' of an aux item, None for raw bytes"""
    if isinstance(item, (bytes, bytearray)):
        return None
    if len(item) == 2:
        return "Z"
    return "B" + item[2][0] if item[1] == "B" else item[1]


def typed_field(rng, kind, tag, count=None):
    """one field of the given kind with a seeded, sometimes hostile value"""
    if kind == "A":
        return (tag, "A", rng.choice("SAOCZ!~ x"))
    if kind in _INT_RANGE:
        lo, hi = _INT_RANGE[kind]
        if kind == "I" and rng.random() < 0.3:
            return (tag, "I", _SAZC)
        return (tag, kind, rng.choice([lo, hi, 0, rng.randint(lo, hi)]))
    if kind == "f":
        return (tag, "f", rng.choice([0.0, -1.5, 3.0e38, rng.random()]))
    if kind == "d":
        return (tag, "d", rng.choice([0.0, struct.unpack("<d", b"SAZchr1,")[0], rng.random()]))
    if kind == "Z":
        return (tag, "Z", rng.choice([b"", b"50A49", DECOY_SA, b"x" + DECOY_OC, bytes(rng.randint(1, 255) for _ in range(rng.randint(1, 40)))]))
    if kind == "H":
        return (tag, "H", rng.choice([b"1AE301", DECOY_SA, DECOY_OC, b"".join(b"%02X" % rng.randint(0, 255) for _ in range(rng.randint(0, 12)))]))
    sub = kind[1]
    n = count if count is not None else (BIG if rng.random() < 0.02 else rng.choice([0, 1, 7]))
    if sub == "C":
        body = bytearray(rng.randbytes(n))
        if n >= len(DECOY_BYTES) and rng.random() < 0.7:
            at = rng.randint(0, n - len(DECOY_BYTES))
            body[at:at + len(DECOY_BYTES)] = DECOY_BYTES
        elif n:
            body[rng.randrange(n)] = 0
        return (tag, "B", ("C", bytes(body)))
    if sub == "f":
        return (tag, "B", ("f", ([0.0, 1.0, -2.5, rng.random()] * (n // 4 + 1))[:n]))
    fmt = {"c": "b", "s": "h", "S": "H", "i": "i", "I": "I"}[sub]
    return (tag, "B", (sub, list(struct.unpack("<%d%s" % (n, fmt), rng.randbytes(n * struct.calcsize(fmt))))))


def bwa_fields(rng):
    """what bwa mem + samtools fixmate leave around SA: (in front, behind)"""
    front = [("NM", "C", rng.randint(0, 9)), ("MD", "Z", "%dA%d" % (rng.randint(1, 60), rng.randint(1, 40))), ("AS", "C", rng.randint(30, 150)),
             ("XS", "C", rng.randint(0, 90))]
    back = [("RG", "Z", "grp%d" % rng.randint(1, 3)), ("MC", "Z", "%dM" % rng.randint(30, 150)), ("MQ", "C", rng.randint(0, 60)),
            ("XA", "Z", "chr3,+%d,100M,1;" % rng.randint(1, 10 ** 6))]
    return front, back


def _names(rng, k):
    # two-letter names that are neither SA nor OC (the second letter never makes one of them)
    return [rng.choice("XYxyzsao") + rng.choice("0123456789bdefghij") for _ in range(k)]


def dress_aux(rng, sa, oc):
    """the aux items of one record: SA / OC where the record has them, typed fields in front, between (both orders) and behind"""
    if not sa:   # most records of a file: the bwa set as it stands, now and then a typed field or an OC without SA (blob stays empty)
        x = rng.getrandbits(32)
        items = [] if x & 7 == 0 else [("NM", "C", x >> 3 & 15), ("MD", "Z", "%dA%d" % (x >> 7 & 63, x >> 13 & 31)), ("AS", "C", x >> 18 & 127), ("XS", "C", x >> 25 & 63),
                                       ("RG", "Z", "grp1"), ("MC", "Z", "%dM" % (30 + (x >> 20 & 127))), ("MQ", "C", x >> 26 & 63)]
        if x >> 30 == 0:
            items.insert(x >> 8 & 3, typed_field(rng, rng.choice(KINDS), _names(rng, 1)[0]))
        if x >> 27 == 11:
            items.append(("OC", "10M"))
        return items
    front, back = bwa_fields(rng)
    if rng.random() < 0.15:
        front, back = [], []
    n_front, n_mid, n_back = rng.randint(3, 6), rng.randint(0, 2), rng.randint(0, 3)
    items = front + [typed_field(rng, rng.choice(KINDS), t) for t in _names(rng, n_front)]
    rng.shuffle(items)
    mid = [typed_field(rng, rng.choice(KINDS), t) for t in _names(rng, n_mid)]
    first = [("SA", sa)] + (mid + [("OC", oc)] if oc else mid)
    if oc and rng.random() < 0.5:
        first = [("OC", oc)] + mid + [("SA", sa)]
    items += first
    if rng.random() < 0.35:   # a second SA behind the first: the first wins
        items.append(("SA", "chr3,777,-,30M70S,20,1;"))
    if oc and rng.random() < 0.35:
        items.append(("OC", "1M99S"))
    tail = back + [typed_field(rng, rng.choice(KINDS), t) for t in _names(rng, n_back)]
    rng.shuffle(tail)
    return items + tail


def dress_body(rng):
    """(packed bases, qualities) of one record"""
    l_seq = rng.choice(L_SEQS)
    seq = rng.randbytes((l_seq + 1) // 2)
    qual = b"\xff" * l_seq if rng.random() < 0.12 else rng.randbytes(l_seq)
    return seq, qual


# ---- hand-written aux layouts -----------------------------------------------------------------------------------------
Layout = namedtuple("Layout", "name qname aux sa oc")
SA1 = "chr2,200000,+,60S40M,60,0;"   # what synth.make_edge's split reads at locus 0 carry
SA2 = "chr3,777,-,30M70S,20,1;"
OC1 = "60M40S"
_ONE = {"A": ("xa", "A", "S"), "c": ("xb", "c", -7), "C": ("xc", "C", 200), "s": ("xd", "s", -30000), "S": ("xe", "S", 65535), "i": ("xf", "i", -2 ** 31),
        "I": ("xg", "I", 2 ** 32 - 1), "f": ("xh", "f", 1.5), "d": ("xi", "d", -2.25), "Z": ("xj", "Z", "text"), "H": ("xk", "H", "1AE301")}
_ARR = {"c": [-1, 2, -3], "C": [1, 2, 3], "s": [-300, 2, 3], "S": [1, 2, 60000], "i": [-70000, 2, 3], "I": [1, 2, 4000000000], "f": [0.5, 1.5, -2.0]}


def _layouts():
    out = []

    def add(name, aux, sa=SA1, oc=""):
        out.append(Layout(name, "lay%02d_%s" % (len(out), name), aux, sa, oc))

    for k in SCALAR_KINDS:
        add("%s_in_front_of_SA" % k, [_ONE[k], ("SA", SA1)])
    add("B_in_front_of_SA", [("xl", "B", ("S", [1, 2, 3])), ("SA", SA1)])
    for s in bamio.AUX_ARRAY_SUBTYPES:
        add("B%s_in_front_of_SA" % s, [("y" + s, "B", (s, _ARR[s])), ("SA", SA1)])
    add("SA_as_last_bytes", [("NM", "C", 1), ("MD", "Z", "60"), ("SA", SA1)])
    add("SA_alone", [("SA", SA1)])
    add("SA_behind_zero_count_B", [("xm", "B", ("i", [])), ("SA", SA1)])
    add("SA_behind_zero_count_BC", [("xm", "B", ("C", b"")), ("SA", SA1)])
    add("empty_Z_in_front_of_SA", [("xn", "Z", ""), ("SA", SA1)])
    add("empty_H_in_front_of_SA", [("xn", "H", ""), ("SA", SA1)])
    add("long_Bi_in_front_of_SA", [("xo", "B", ("i", list(range(-1500, 1501)))), ("SA", SA1)])
    add("long_Bs_behind_SA", [("SA", SA1), ("xo", "B", ("s", [7] * BIG))])
    add("decoy_I_spells_SAZc", [("xp", "I", _SAZC), ("SA", SA1)])
    add("decoy_I_spells_SAZc_no_SA", [("xp", "I", _SAZC), ("xq", "Z", "chr2,5,+,60S40M,60,0;")], sa="")
    add("decoy_in_Z", [("xr", "Z", b"q" + DECOY_SA), ("SA", SA1)])
    add("decoy_in_Z_no_SA", [("xr", "Z", b"q" + DECOY_SA), ("xs", "Z", b"q" + DECOY_OC)], sa="")
    add("decoy_in_H", [("xt", "H", DECOY_SA), ("OC", OC1), ("SA", SA1)], oc=OC1)
    add("decoy_in_BC", [("xu", "B", ("C", b"\1" + DECOY_BYTES + b"\2")), ("SA", SA1)])
    add("decoy_in_BC_no_SA", [("xu", "B", ("C", DECOY_BYTES))], sa="")
    add("B_payload_of_NULs", [("xv", "B", ("C", bytes(9))), ("xw", "B", ("I", [0, 0])), ("SA", SA1)])
    add("OC_before_SA", [("NM", "C", 0), ("OC", OC1), ("AS", "C", 60), ("SA", SA1), ("RG", "Z", "g")], oc=OC1)
    add("OC_after_SA", [("NM", "C", 0), ("SA", SA1), ("AS", "C", 60), ("OC", OC1), ("RG", "Z", "g")], oc=OC1)
    add("OC_without_SA", [("NM", "C", 0), ("OC", OC1)], sa="")
    add("double_SA", [("SA", SA1), ("xx", "c", 0), ("SA", SA2)])
    add("double_OC", [("OC", OC1), ("SA", SA1), ("OC", "1M99S")], oc=OC1)
    add("bwa_set", [("NM", "C", 2), ("MD", "Z", "10A49"), ("AS", "C", 55), ("XS", "C", 20), ("SA", SA1), ("RG", "Z", "grp1"), ("MC", "Z", "100M"), ("MQ", "C", 60),
                    ("XA", "Z", "chr3,+500,100M,1;")])
    # out of the SAM specification, pinned to what the reference does with them
    add("SA_of_type_H", [("SA", "H", SA1)])
    add("OC_of_type_H", [("OC", "H", OC1), ("SA", SA1)], oc=OC1)
    add("SA_of_type_A_hides_SA_Z", [b"SAAx", ("SA", SA1)], sa="xSAZ" + SA1)
    add("SA_of_type_C_zero_hides_SA_Z", [b"SAC\0", ("SA", SA1)], sa="")
    add("empty_SA_hides_SA_Z", [("SA", ""), ("SA", SA1)], sa="")
    add("Bd_in_front_of_SA", [b"xyBd" + struct.pack("<I", 3) + bytes(12) + b"SAZchr4,9,+\0", ("SA", SA1)])
    return out


LAYOUTS = _layouts()
LONG_NAME = "L" * 254   # l_read_name = 255: one discordant pair, both mates dressed
LAYOUT_REGION = ("chr1", 98_669, 101_331)   # holds the primary of every layout read


def layout_recs():
    """the reads of LAYOUTS as synth records (a split-read triple each, at locus 0 of synth.make_edge) + the long-named pair"""
    recs = []
    for lay in LAYOUTS:
        prim = synth.Rec(lay.qname, 0x1 | 0x2 | 0x40 | 0x20, 0, 99_950, 60, "55M45S" if lay.oc else "60M40S", 0, 100_100, 250, sa=lay.sa, oc=lay.oc)
        part = synth.Rec(lay.qname, 0x1 | 0x40 | 0x20 | 0x100, 1, 199_999, 60, "60S40M", 0, 100_100, 0, sa="chr1,99951,+,60M40S,60,0;")
        mate = synth.Rec(lay.qname, 0x1 | 0x2 | 0x80 | 0x10, 0, 100_100, 60, "100M", 0, 99_950, -250)
        recs += [prim, part, mate]
    recs += synth._discordant_pair(LONG_NAME, 0, 100_020, 1, 200_020, 100)
    return recs


def with_layouts(ds):
    """ds + the layout reads, coordinate sorted"""
    out = synth.Dataset(list(ds.contigs), list(ds.recs) + layout_recs())
    out.sort()
    return out


def dress_plan(ds, seed=_SEED):
    """[(record, packed bases, qualities, aux items)] of a Dataset; the primary of a layout read gets its layout's aux"""
    rng = random.Random(seed)
    by_name = {lay.qname: lay for lay in LAYOUTS}
    plan = []
    for r in ds.recs:
        seq, qual = dress_body(rng)
        aux = dress_aux(rng, r.sa, r.oc)
        lay = by_name.get(r.qname)
        if lay is not None and r.flag & 0x40 and not r.flag & 0x900:
            aux = lay.aux
        plan.append((r, seq, qual, aux))
    return plan


def encode_plan(plan):
    for r, seq, qual, aux in plan:
        yield bamio.encode_record(r.qname, r.flag, r.tid, r.pos, r.mapq, bamio.parse_cigar(r.cigar), r.mtid, r.mpos, r.isize, aux, seq=seq, qual=qual)


def dressed_records(ds, seed=_SEED):
    """the encoded records of a synth.Dataset, dressed"""
    return encode_plan(dress_plan(ds, seed))


def write_dressed(ds, path, seed=_SEED, aligned=False):
    bamio.write_bam(path, ds.contigs, dressed_records(ds, seed), aligned=aligned)


def kinds_in_front_of_sa(aux):
    """the kinds of the typed fields that stand in front of the first SA:Z of an aux item list"""
    out = []
    for it in aux:
        if not isinstance(it, (bytes, bytearray)) and it[0] == "SA" and kind_of(it) == "Z":
            return out
        if kind_of(it) is not None:
            out.append(kind_of(it))
    return []


def edge_dressed():
    """the Dataset behind tests/golden/edge_dressed.* (tools/make_golden.py: dressed_datasets)"""
    return with_layouts(synth.make_edge())


# ---- a payload that looks like records, where a boundary guess looks first ---------------------------------------------
BLOCK = 0xFF00        # bamio.write_bam cuts the inflated stream of a file with records across blocks every BLOCK bytes
DECOY_CHAIN = 6       # more than GUESS_CHAIN (bam_gpu.hip) well-formed minimal records in a row
_DECOY_REC = struct.pack("<iiiBBHHHIiii", 34, 0, 0, 2, 0, 4680, 0, 0, 0, -1, -1, 0) + b"d\0"


def write_decoy_chain_file(ds, path, ends_with_record, seed=_SEED):
    """ds, dressed, with records across blocks; one record in the middle carries a B:C array longer than a BGZF block whose
    bytes hold DECOY_CHAIN well-formed minimal records, the first of them at the first byte of a block.  ends_with_record:
    the chain's last byte is the record's last byte (the walk of the decoys runs on into the real records); otherwise more
    than a block of filler follows.  Legal BAM: the expected table is ds.to_soa().  Returns the block the chain starts."""
    recs = list(dressed_records(ds, seed))
    t = ("@HD\tVN:1.4\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in ds.contigs)).encode()
    start = 12 + len(t) + sum(4 + len(n) + 1 + 4 for n, _ in ds.contigs)
    i = len(recs) // 2
    start += sum(len(r) for r in recs[:i])
    payload_at = start + len(recs[i]) + 3 + 1 + 4   # the array goes behind the record's own fields
    k = -(-payload_at // BLOCK) + (1 if ends_with_record else 0)
    chain = _DECOY_REC * DECOY_CHAIN
    payload = b"\xAA" * (k * BLOCK - payload_at) + chain + (b"" if ends_with_record else b"\xAA" * (BLOCK + 4321))
    assert len(payload) > BLOCK
    body = recs[i][4:] + b"zzBC" + struct.pack("<I", len(payload)) + payload
    recs[i] = struct.pack("<i", len(body)) + body
    bamio.write_bam(path, ds.contigs, recs, header_text=t.decode())
    # the file as written: the chain lies where it was aimed (were the header or the cuts to drift, the test would go vacuous)
    stream = bamio.inflate(path)
    head, got = bamio.read_records(path)
    end = len(head) + sum(4 + len(r) for r in got[:i + 1])
    assert got == [r[4:] for r in recs] and stream[k * BLOCK:k * BLOCK + len(chain)] == chain
    assert (end == k * BLOCK + len(chain)) if ends_with_record else (end == k * BLOCK + len(chain) + BLOCK + 4321)
    assert end // BLOCK == k or not ends_with_record   # the chain's record ends inside the block the chain starts
    return k
