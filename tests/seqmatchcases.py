"""Shared cases of the sequence-match tests (test_cpu_seqmatch, test_gpu_seqmatch, test_gpu_lociseq): the definition of
bk_sequence_match (include/breakid_hip.h) as a brute force over every diagonal of every sequence in both orientations, with no index;
the FASTA reader of `-panel` for expected files; and drawn panels and queries."""
import numpy as np

from breakid_amd import abi

CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGTN"):
    CODE[_c] = _i
PAD = 256  # bases between two sequences of the laid-out panel: more than a query is long, so no diagonal meets two sequences
GAP = 5    # the code of those bases: it equals no query code


def codes_of(s):
    """str / bytes of A C G T N -> codes 0..4"""
    b = s.encode() if isinstance(s, str) else bytes(s)
    c = CODE[np.frombuffer(b, np.uint8)]
    assert (c <= 4).all(), s
    return c


def revcomp_codes(c):
    return np.where(c < 4, 3 - c, c)[::-1]


class Panel:
    """the sequences laid out in one array with PAD bases of GAP around each"""

    def __init__(self, seqs):
        self.seqs = [codes_of(s) for s in seqs]
        self.lens = [len(c) for c in self.seqs]
        parts, self.start, at = [np.full(PAD, GAP, np.uint8)], [], PAD
        for c in self.seqs:
            self.start.append(at)
            parts += [c, np.full(PAD, GAP, np.uint8)]
            at += len(c) + PAD
        self.cat = np.concatenate(parts)
        self.sid = np.full(len(self.cat), -1, np.int64)  # the sequence whose diagonals start at x: x in [start - PAD + 1, start + len)
        for s, (a, n) in enumerate(zip(self.start, self.lens)):
            self.sid[a - PAD + 1:a + n] = s

    def arrays(self):
        """(off, bases) as bk_seq_panel takes them"""
        off = np.cumsum([0] + self.lens).astype(np.uint64)
        bases = np.frombuffer(b"ACGTN", np.uint8)[np.concatenate(self.seqs)] if sum(self.lens) else np.zeros(0, np.uint8)
        return off, np.ascontiguousarray(bases)

    def kmers(self, seed):
        """M of the byte model: the positions whose `seed` bases hold no N and end inside their sequence"""
        m = 0
        for c in self.seqs:
            if len(c) >= seed:
                bad = np.concatenate([[0], np.cumsum(c >= 4)])
                m += int((bad[seed:] - bad[:-seed] == 0).sum())
        return m


def seeded_diagonals(panel, q, seed):
    """Every diagonal of every sequence against q (codes): diagonal x holds the cells q[i] against cat[x + i].  Returns (the x of the
    diagonals with a run of at least `seed` cells, the number of such runs)."""
    L = len(q)
    nx = len(panel.cat) - L + 1
    cur = np.zeros(nx, np.int16)
    seeded = np.zeros(nx, bool)
    n_seeds = 0
    for i in range(L):
        if q[i] >= 4:
            cur[:] = 0
            continue
        m = panel.cat[i:i + nx] == q[i]
        cur += 1
        cur *= m
        hit = cur == seed  # a run of at least `seed` cells passes through here once
        n_seeds += int(np.count_nonzero(hit))
        seeded |= hit
    return np.flatnonzero(seeded), n_seeds


def scan(panel, q, x, s):
    """The one pass over diagonal x of sequence s: (the offers (score, n, i0, d) of every matching cell, the longest run)"""
    d = int(x) - panel.start[s]
    P, n_s = panel.seqs[s], panel.lens[s]
    total = since = cur = run = 0
    offers = []
    for i in range(len(q)):
        if not 0 <= i + d < n_s:
            continue
        if q[i] < 4 and q[i] == P[i + d]:
            if total <= 0:
                total = since = 0
            total, since, cur = total + 1, since + 1, cur + 1
            run = max(run, cur)
            offers.append((total, since, i + 1 - since, d))
        else:
            total, since, cur = total - 2, since + 1, 0
    return offers, run


def match_one(panel, text, reversed_, seed):
    """one abi.SEQ_HIT row as a dict"""
    q = codes_of(text)
    if reversed_:
        q = q[::-1]
    row = dict(found=0, seq=-1, orient=0, score=0, len=0, mism=0, run=0, q_start=0, s_start=0, n_seeds=0, seq2=-1, score2=0)
    if len(q) == 0 or not panel.seqs:
        return row
    best, run, n_seeds, per_seq = None, 0, 0, {}
    for o, qo in enumerate((q, revcomp_codes(q))):
        xs, ns = seeded_diagonals(panel, qo, seed)
        n_seeds += ns
        for x in xs:
            s = int(panel.sid[x])
            assert s >= 0
            offers, r = scan(panel, qo, x, s)
            run = max(run, r)
            for score, n, i0, d in offers:
                key = (score, -n, -s, -o, -(i0 + d), -i0)
                if best is None or key > best:
                    best = key
                per_seq[s] = max(per_seq.get(s, 0), score)
    if n_seeds == 0:
        return row
    score, n, s, o, s_start, i0 = best[0], -best[1], -best[2], -best[3], -best[4], -best[5]
    row.update(found=1, seq=s, orient=o, score=score, len=n, mism=(n - score) // 3, run=run, q_start=(len(q) - i0 - n) if o else i0, s_start=s_start, n_seeds=n_seeds)
    others = {t: v for t, v in per_seq.items() if t != s}
    if others:
        row["score2"] = max(others.values())
        row["seq2"] = min(t for t, v in others.items() if v == row["score2"])
    return row


def expected_hits(seqs, queries, seed, reversed_=None):
    """abi.SEQ_HIT rows of `queries` (str; as the bytes lie in the query array) against the sequences `seqs` (str) or a Panel"""
    panel = seqs if isinstance(seqs, Panel) else Panel(seqs)
    out = np.zeros(len(queries), abi.SEQ_HIT)
    for k, text in enumerate(queries):
        r = match_one(panel, text, bool(reversed_[k]) if reversed_ is not None else False, seed)
        for f in abi.SEQ_HIT.names:
            out[k][f] = r[f]
    return out


def pack(queries, max_len=None, reversed_=None):
    """(abi.SEQ_PROBE rows, uint8 [n, max_len]) of the str `queries`; the bytes behind qlen are 0"""
    max_len = max_len or max([len(t) for t in queries] + [1])
    probes = np.zeros(len(queries), abi.SEQ_PROBE)
    query = np.zeros((len(queries), max_len), np.uint8)
    for k, t in enumerate(queries):
        probes[k] = (len(t), int(reversed_[k]) if reversed_ is not None else 0)
        query[k, :len(t)] = np.frombuffer(t.encode(), np.uint8)
    return probes, query


def revcomp(t):
    return t.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def draw(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def mutate(rng, t, rate):
    """substitutions at `rate`: each chosen base becomes one of the three others"""
    out = list(t)
    for i in np.flatnonzero(rng.random(len(t)) < rate):
        out[i] = "ACGT"[("ACGT".index(out[i]) + int(rng.integers(1, 4))) % 4] if out[i] in "ACGT" else out[i]
    return "".join(out)


def drawn_panel(rng, n_seqs=40, total=70000, tail=True):
    """about `total` drawn bases in n_seqs sequences of uneven length, a poly-A tail of 10 to 30 on every other one"""
    cuts = np.sort(rng.integers(200, total - 200, n_seqs - 1))
    lens = np.diff(np.concatenate([[0], cuts, [total]]))
    return [draw(rng, int(n)) + ("A" * int(rng.integers(10, 31)) if tail and s % 2 else "") for s, n in enumerate(lens)]


def cut_queries(rng, seqs, n, qlen, rate):
    """n queries of qlen bases cut from the sequences that are long enough, every other one reverse-complemented, mutated at `rate`"""
    long_enough = [s for s, t in enumerate(seqs) if len(t) >= qlen]
    out = []
    for k in range(n):
        t = seqs[long_enough[int(rng.integers(0, len(long_enough)))]]
        a = int(rng.integers(0, len(t) - qlen + 1))
        piece = mutate(rng, t[a:a + qlen], rate)
        out.append(revcomp(piece) if k % 2 else piece)
    return out


# ---- the FASTA of -panel -----------------------------------------------------------------------------------------------------------------
def read_fasta(path):
    """(names, sequences) by the rules of `-panel`: a `>` line names a sequence by its first word, bases are upper-cased, every letter
    other than A C G T becomes N, blank lines are skipped.  ValueError("line N: ...") for sequence data before a header, a duplicate
    name and a sequence without bases."""
    names, seqs, at = [], [], []
    with open(path, "rb") as f:
        for no, raw in enumerate(f.read().split(b"\n"), 1):
            line = raw.strip().decode("latin-1")
            if not line:
                continue
            if line.startswith(">"):
                if names and not seqs[-1]:
                    raise ValueError("line %d: sequence %s has no bases" % (at[-1], names[-1]))
                word = line[1:].split()
                name = word[0] if word else ""
                if not name:
                    raise ValueError("line %d: a header without a name" % no)
                if name in names:
                    raise ValueError("line %d: duplicate sequence name %s" % (no, name))
                names.append(name)
                seqs.append("")
                at.append(no)
            else:
                if not names:
                    raise ValueError("line %d: sequence data before the first header" % no)
                seqs[-1] += "".join(c if c in "ACGT" else "N" for c in line.upper())
    if names and not seqs[-1]:
        raise ValueError("line %d: sequence %s has no bases" % (at[-1], names[-1]))
    return names, seqs


HAND_PANEL = ["GGCCGGGCGCGGTGGCTCACGCCTGTAATCCCAGCA", "TTGACCATGGCTAGCATCGGATTACAGGCGTGAGCCACCAAAAAAAAAAAA", "GGCCGGGCGCGGTGGCTCATGCCTGTAAT"]
