"""Shared by tests/test_left_align_gpu.py and tests/test_left_align_host.py: a genome with planted homopolymers and tandem
repeats (on the contigs and helpers of tests/candidates_reference_cases.py), reads on it given as (start, end, edits), and for
every read its TWIN: the same SEQ with every eligible insertion and deletion placed where the Python restatement of the rule
(``dl4vc_amd.truthset.left_align_letters``) puts it, with the read's own start as the floor; CIGAR and MD are rebuilt.  The
oracle of the GPU tests is "BAM X with the option == twin BAM X' without it": VCF body byte for byte, tuples equal as doubles.

Shifting a deletion changes which positions the twin's CIGAR covers, so DP is equal only where no allele of any read lies inside
a shifted window [a - k + 1, a + L]: ``build`` asserts that for the fixture (a condition of the fixture, not a tolerance).  Also
here: the counters the restatement expects over the fetched reads, and the enumerated grid of the host test and the sanitizer
program (contigs of 1..12 bases over {A, C, N}, every anchor, L in 1..4, both kinds, every floor)."""
import itertools

from dl4vc_amd import truthset as T
from dl4vc_amd.bamio import CMATCH, CINS, CDEL, CSOFT_CLIP
from tests import candidates_reference_cases as K

NAMES = [c[0] for c in K.CONTIGS]
MAX_LEN = 60
THRESHOLD_POS = 1499          # ctgB, 0-based: the event that passes --indel_min_freq 0.02 only as a whole
BED = "ctgA\t2000\t2100\n"


def _other(b):
    return "ACGT"[("ACGT".index(b) + 1) % 4] if b in "ACGT" else "A"


def make_genome():
    """The seeded genome of the reference cases without its special bytes, with the repeats of the cases written in."""
    g = K.make_genome(special=False)
    a, b = g["ctgA"], g["ctgB"]
    def put(contig, at, text):
        contig[at:at + len(text)] = text.encode()
    put(a, 0, "GAAAAAAC")                               # a shift that reaches position 0
    put(a, 199, "G" + "T" * 8 + "C")                    # homopolymer: three placements of one deletion
    put(a, 399, "G" + "AC" * 6 + "T")                   # tandem repeat: deletions of 2 and 4
    put(a, 599, "G" + "AC" * 6 + "T")                   # tandem repeat: insertions, rotated, and a shift > L
    put(a, 799, "G" + "A" * 10 + "C")                   # a read that starts inside
    put(a, 995, "G" + "T" * 10 + "C")                   # across the subregion boundary at 1000
    put(a, 1995, "G" + "T" * 10 + "C")                  # inside a BED interval [2000, 2100], shifts out of it
    put(a, 2096, "G" + "A" * 10 + "C")                  # outside it, shifts in
    put(a, 2300, "G" + "AAAANAAAAA" + "C")              # N stops the shift
    put(a, 2400, "G" + "TTTTRTTTTT" + "C")              # an IUPAC code stops the shift
    put(a, 2599, "G" + "A" * 6 + "C")                   # the MD that names other deleted bases
    put(a, 2700, "T" * 10 + "C")                        # leading deletion
    put(a, 2929, "G" + "A" * 6 + "C")                   # an insertion directly behind a deletion
    for at, n, shifts in ((3100, 59, True), (3300, 60, True), (3500, 59, False), (3700, 60, False)):
        put(a, at - 1, "AG")                            # REF of 60 kept, of 61 dropped; shiftable by exactly one base, or not
        put(a, at + n - 1, "CG" if shifts else "CT")
    put(b, 1499, "G" + "A" * 8 + "C")                   # the threshold case
    return g


# ---- reads ----------------------------------------------------------------------------------------------------------------------
def build_read(ref, start, end, edits):
    """A read over ref[start, end) with ``edits``: ("D", a, L) deletes ref[a + 1 .. a + L], ("I", a, bases) inserts behind a,
    ("X", p, base) substitutes.  Returns (cigar, seq); a reference letter outside ACGT reads as A."""
    by = {}
    for e in edits:
        assert e[1] not in by and start <= e[1] < end
        by[e[1]] = e
    ops, seq, p = [], [], start
    def push(op, n):
        if ops and ops[-1][0] == op:
            ops[-1][1] += n
        else:
            ops.append([op, n])
    while p < end:
        e = by.get(p)
        b = ref[p] if ref[p] in "ACGT" else "A"
        seq.append(e[2] if e and e[0] == "X" else b)
        push(CMATCH, 1)
        if e and e[0] == "I":
            seq.append(e[2])
            push(CINS, len(e[2]))
        elif e and e[0] == "D":
            push(CDEL, e[2])
            p += e[2]
        p += 1
    assert p == end and ops[-1][0] == CMATCH and ops[0][0] == CMATCH
    return [tuple(o) for o in ops], "".join(seq)


def _place(ref, start, e):
    """The edit where the rule puts it, and (k, eligible, clamped)."""
    if e[0] == "X":
        return e, (0, True, False)
    kind = T.LA_DEL if e[0] == "D" else T.LA_INS
    bases = ref[e[1] + 1:e[1] + 1 + e[2]] if e[0] == "D" else e[2]
    anchor = ref[e[1]] if ref[e[1]] in "ACGT" else "A"
    p, _, s, ok, clamped = T.left_align_letters(lambda i: ref[i], len(ref), kind, e[1], anchor, bases, start)
    return ((e[0], p, e[2]) if e[0] == "D" else (e[0], p, s)), (e[1] - p, ok, clamped)


def _read(tid, pos, cigar, seq, md, obs):
    return dict(tid=tid, pos=pos, flag=0, cigar=cigar, seq=seq, md=md, obs=obs)


def build(md=True):
    """``dict(genome, x, twin, windows)``: the reads of BAM X and of its twin X' (coordinate order, same names), each with
    ``obs``: its indel observations as (kind, a, anchor, bases, anchor_aligned, counted) for the expected counters.  ``md``
    False: the reads are for BAMs without MD tags (the read whose MD disagrees with the FASTA is left out)."""
    genome = make_genome()
    refs = {n: K.rule_letters(bytes(genome[n])) for n in NAMES}
    x, twin, windows = [], [], []

    def add(tid, start, end, edits):
        ref = refs[NAMES[tid]]
        placed = [_place(ref, start, e) for e in edits]
        cig, seq = build_read(ref, start, end, edits)
        tcig, tseq = build_read(ref, start, end, [p[0] for p in placed])
        assert seq == tseq, (start, edits)                                    # the defining property
        obs = []
        for e, (pe, (k, ok, _)) in zip(edits, placed):
            if e[0] == "X":
                continue
            L = e[2] if e[0] == "D" else len(e[2])
            bases = ref[e[1] + 1:e[1] + 1 + L] if e[0] == "D" else e[2]
            obs.append((T.LA_DEL if e[0] == "D" else T.LA_INS, e[1], ref[e[1]] if ref[e[1]] in "ACGT" else "A", bases, True, True))
            if k:
                windows.append((tid, e[1] - k + 1, e[1] + (L if e[0] == "D" else 0)))
        x.append(_read(tid, start, cig, seq, K.md_for(ref, start, cig, seq), obs))
        twin.append(_read(tid, start, tcig, tseq, K.md_for(ref, start, tcig, tseq), None))

    def raw(tid, pos, cigar, seq, obs, md_text=None):
        """A read given as it is, whose twin is itself: nothing of it may shift."""
        ref = refs[NAMES[tid]]
        for kind, a, anchor, bases, aligned, counted in obs:
            p = T.left_align_letters(lambda i: ref[i], len(ref), kind, a, anchor, bases, pos, aligned)[0]
            assert p == a or md_text is not None
        r = _read(tid, pos, cigar, seq, md_text or K.md_for(ref, pos, cigar, seq), obs)
        x.append(r)
        twin.append(dict(r, obs=None))

    A = refs["ctgA"]
    def m(a, n):
        return "".join(c if c in "ACGT" else "A" for c in A[a:a + n])
    # position 0
    add(0, 0, 80, [("D", 4, 1)])
    add(0, 0, 80, [("X", 30, _other(A[30]))])
    # one deletion of a homopolymer at three placements, and two plain reads
    for start, a in ((150, 199), (160, 201), (170, 203)):
        add(0, start, start + 100, [("D", a, 1)])
    add(0, 155, 255, [])
    add(0, 165, 265, [("X", 230, _other(A[230]))])
    # ACACAC: deletions of 2 and 4 bases
    add(0, 340, 440, [("D", 405, 2)])
    add(0, 345, 445, [("D", 399, 2)])
    add(0, 350, 450, [("D", 403, 4)])
    add(0, 355, 455, [])
    # ACACAC: CA behind an A and AC behind a C are one insertion; ACAC shifts by 10 > L = 4
    add(0, 540, 640, [("I", 604, "CA")])
    add(0, 545, 645, [("I", 607, "AC")])
    add(0, 550, 650, [("I", 609, "ACAC")])
    add(0, 555, 655, [])
    # a read that starts inside the repeat keeps a placement of its own
    add(0, 803, 900, [("D", 806, 1)])
    add(0, 750, 850, [("D", 799, 1)])
    add(0, 760, 860, [])
    # across position 1000
    add(0, 950, 1050, [("D", 1002, 1)])
    add(0, 940, 1040, [("D", 995, 1)])
    add(0, 960, 1060, [("X", 1030, _other(A[1030]))])
    # around the BED interval [2000, 2100]
    add(0, 1950, 2050, [("D", 2003, 1)])
    add(0, 1960, 2060, [])
    add(0, 2050, 2150, [("D", 2103, 1)])
    add(0, 2060, 2160, [("X", 2080, _other(A[2080]))])
    # N and an IUPAC code inside the repeat
    add(0, 2250, 2350, [("D", 2308, 1)])
    add(0, 2255, 2355, [])
    add(0, 2350, 2450, [("D", 2408, 1)])
    add(0, 2355, 2455, [])
    # the MD names a deleted C where the FASTA has an A: not eligible, not shifted
    if md:
        raw(0, 2550, [(CMATCH, 53), (CDEL, 1), (CMATCH, 40)], m(2550, 53) + m(2604, 40), [(T.LA_DEL, 2602, "A", "C", True, True)],
            md_text="53^C40")
    add(0, 2555, 2655, [])
    # S D M: the deletion takes the read's last pair as its anchor
    raw(0, 2700, [(CSOFT_CLIP, 5), (CDEL, 3), (CMATCH, 60)], "GGGGG" + m(2703, 60), [(T.LA_DEL, 2762, A[2762], A[2700:2703], False, True)])
    # I then D: the read's deletions are dropped; its insertion cannot shift
    ins = _other(A[2829]) * 2
    raw(0, 2800, [(CMATCH, 30), (CINS, 2), (CDEL, 3), (CMATCH, 30)], m(2800, 30) + ins + m(2833, 30),
        [(T.LA_INS, 2829, A[2829], ins, True, True), (T.LA_DEL, 2829, A[2829], A[2830:2833], False, False)])
    # D then I: the insertion is anchored on the deleted position (in a homopolymer, where an aligned anchor would shift)
    raw(0, 2900, [(CMATCH, 30), (CDEL, 1), (CINS, 1), (CMATCH, 40)], m(2900, 30) + "A" + m(2931, 40),
        [(T.LA_DEL, 2929, "G", "A", True, True), (T.LA_INS, 2930, "A", "A", False, True)])
    # REF of 60 bases kept, of 61 dropped, shifted by one base or not
    for at, n in ((3100, 59), (3300, 60), (3500, 59), (3700, 60)):
        for k in range(2):
            add(0, at - 40 - k, at + n + 31, [("D", at, n)])
    # the threshold case: 60 reads over the homopolymer, one deletion at two placements
    for i in range(60):
        add(1, 1440 + i % 30, 1540 + i % 30, [("D", 1501, 1)] if i == 0 else [("D", 1503, 1)] if i == 1 else [])
    for i, (r, t) in enumerate(zip(x, twin)):
        r["name"] = t["name"] = "q%d" % i
    order = sorted(range(len(x)), key=lambda i: (x[i]["tid"], x[i]["pos"]))
    x, twin = [x[i] for i in order], [twin[i] for i in order]
    # the fixture's condition: no allele of any read of the twin inside a shifted window
    for t in twin:
        p = t["pos"]
        q = 0
        for op, n in t["cigar"]:
            if op == CMATCH:
                ref = refs[NAMES[t["tid"]]]
                for i in range(n):
                    if t["seq"][q + i] != (ref[p + i] if ref[p + i] in "ACGT" else "A"):
                        assert not [w for w in windows if w[0] == t["tid"] and w[1] <= p + i <= w[2]], (t["name"], p + i)
                p += n
                q += n
            elif op == CDEL:
                assert not [w for w in windows if w[0] == t["tid"] and w[1] <= p - 1 <= w[2]], (t["name"], p - 1)
                p += n
            elif op in (CINS, CSOFT_CLIP):
                if q:
                    assert not [w for w in windows if w[0] == t["tid"] and w[1] <= p - 1 <= w[2]], (t["name"], p - 1)
                q += n
    return dict(genome=genome, refs=refs, x=x, twin=twin, windows=windows)


def span(r):
    return sum(n for op, n in r["cigar"] if op in (CMATCH, CDEL)) or 1


def expected_counters(case, subregions):
    """The five counters over the reads a run over ``subregions`` ((contig, start, end)) fetches from BAM X: every indel
    observation that is counted as an allele (length and drop rule as without the option, lo <= shifted position <= hi)."""
    c = dict(observations=0, shifted=0, bases_shifted=0, clamped=0, not_eligible=0)
    for r in case["x"]:
        ref = case["refs"][NAMES[r["tid"]]]
        for contig, s, e in subregions:
            if contig != NAMES[r["tid"]] or not (r["pos"] < e and r["pos"] + span(r) > s):
                continue
            for kind, a, anchor, bases, aligned, counted in r["obs"]:
                if not counted or len(bases) + 1 > MAX_LEN:
                    continue
                p, _, _, ok, clamped = T.left_align_letters(lambda i: ref[i], len(ref), kind, a, anchor, bases, r["pos"], aligned)
                if not s <= p <= e:
                    continue
                c["observations"] += 1
                c["shifted"] += p != a
                c["bases_shifted"] += a - p
                c["clamped"] += clamped
                c["not_eligible"] += not ok
    return c


def observations(case):
    """Every observation of the fixture as the arguments of the rule: (letters, kind, a, anchor, bases, floor, aligned)."""
    return [(case["refs"][NAMES[r["tid"]]], kind, a, anchor, bases, r["pos"], aligned)
            for r in case["x"] for kind, a, anchor, bases, aligned, _ in r["obs"]]


def grid():
    """The enumerated grid: contigs of 1..12 bases over {A, C, N} (all of them up to 5 bases, about 30 seeded ones per length
    beyond: tools/asan_left_align.sh runs the full grid in C++), every anchor, L in 1..4, both kinds, every floor (three of
    them beyond 5 bases); the inserted bases run over {A, C} words, the deleted ones are the contig's."""
    import random
    rng = random.Random(5)
    for n in range(1, 13):
        for letters in itertools.product("ACN", repeat=n):
            if n > 5 and rng.random() > 30.0 / 3 ** n:
                continue
            g = "".join(letters)
            for a in range(n):
                for L in range(1, 5):
                    floors = range(0, a + 1) if n <= 5 else (0, a // 2, a)
                    for floor in floors:
                        yield g, T.LA_DEL, a, g[a], g[a + 1:a + 1 + L].ljust(L, "A"), floor
                        for word in sorted({"A" * L, ("AC" * L)[:L], ("CA" * L)[:L], ("CCA" * L)[:L]}):
                            yield g, T.LA_INS, a, g[a], word, floor


def write_case(case, directory, md=True):
    """``(x_bam, twin_bam)`` in ``directory``."""
    md_of = K.with_md if md else K.without_md
    return (K.write_bam(str(directory / ("x%d.bam" % md)), case["x"], md_of),
            K.write_bam(str(directory / ("twin%d.bam" % md)), case["twin"], md_of))
