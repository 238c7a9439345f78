"""Inputs and expected values for the graph kernels at sizes where their loops take a second trip (tests/test_gpu_graph_sizes.py; pinned without a device by
tests/test_graph_sizes_cpu.py). Two parts.

A FAST STATEMENT for k <= 31 (one uint64 per k-mer) of what tests/test_graph_cpu.py, test_unitigs_cpu.py and test_unitig_links_cpu.py state record by record in Python:
neighbour masks, topology, branching records, record links, unitigs (bases, offsets, KC, per record the unitig, reversed flag and position) and the unitig-link CSR, over
all records or over an ``alive`` subset (dead records: mask 0, no unitig, named by no mask — the contract of gkc_graph_unitigs_build_alive). It states the DEFINITION in
numpy: a neighbour is present when a binary search of the sorted canonical values finds it; paths are walked from their end records, one step at a time (all paths in
lock step while there are many, the few long ones in a plain loop), cycles from their smallest record. No pointer jumping, no tile scan, no minimizers: it shares nothing
with csrc/gkc_graph.hip and csrc/gkc_unitigs.hip. 2 * 10^6 records take seconds where the Python statements take minutes.

CONSTRUCTIONS whose record count, unitig count and simplification are known from how they are made: isolated paths, one long path, one long circle, padding plus
branching structures (forks, tips, SNP bubbles, erroneous connections), and isolated paths at k = 33 with a closed-form answer. Every construction counts its distinct
canonical k-mers and (k-1)-mers with np.unique, which is what makes its n exact; a seed that fails gives way to the next in a bounded loop that raises at its end.

Nucleotide codes: A, C, T, G = 0..3 (the complement is ^ 2)."""
import numpy as np

NONE = -1
LETTERS = np.frombuffer(b"ACTG", np.uint8)
_POP4 = np.array([bin(i).count("1") for i in range(16)], np.uint8)
_LOG2 = np.array([max(i.bit_length() - 1, 0) for i in range(16)], np.uint64)
_U = np.uint64


# ------------------------------------------------------------------------------------------------ the fast statement: k-mers as uint64
def revcomp_np(x, k):
    """reverse complement of k-mers (k <= 32) held as uint64: every nucleotide complemented, the 32 two-bit groups reversed, the unused ones shifted out"""
    x = np.asarray(x, np.uint64) ^ _U(0xAAAAAAAAAAAAAAAA)
    x = ((x >> _U(2)) & _U(0x3333333333333333)) | ((x & _U(0x3333333333333333)) << _U(2))
    x = ((x >> _U(4)) & _U(0x0F0F0F0F0F0F0F0F)) | ((x & _U(0x0F0F0F0F0F0F0F0F)) << _U(4))
    return x.byteswap() >> _U(64 - 2 * k)


def neighbour_np(x, k, e):
    """neighbour e (0-3: right extension by A, C, T, G; 4-7: left extension) of x taken as the forward strand; e a number or an array"""
    e = np.asarray(e, np.uint64)
    right = ((x << _U(2)) | (e & _U(3))) & _U((1 << (2 * k)) - 1)
    left = (x >> _U(2)) | ((e & _U(3)) << _U(2 * (k - 1)))
    return np.where(e < _U(4), right, left)


class Lookup:
    """canonical value -> flat record index, over the alive records: a binary search of the sorted values"""

    def __init__(self, values, alive=None):
        idx = np.arange(len(values)) if alive is None else np.flatnonzero(alive)
        o = np.argsort(values[idx], kind="stable")
        self.sv, self.si = values[idx][o], idx[o]
        assert len(self.sv) < 2 or (self.sv[1:] != self.sv[:-1]).all(), "the values are distinct"

    def find(self, keys):
        """-> (found bool[], flat index int64[] where found)"""
        if not len(self.sv):
            return np.zeros(len(keys), bool), np.zeros(len(keys), np.int64)
        p = np.minimum(np.searchsorted(self.sv, keys), len(self.sv) - 1)
        return self.sv[p] == keys, self.si[p]


def masks_fast(values, k, alive=None, lookup=None):
    """uint8[n]: bit e set <=> the canonical form of neighbour e is an alive record; 0 for dead records"""
    values = np.asarray(values, np.uint64)
    lookup = lookup or Lookup(values, alive)
    out = np.zeros(len(values), np.uint8)
    for e in range(8):
        y = neighbour_np(values, k, e)
        found, _ = lookup.find(np.minimum(y, revcomp_np(y, k)))
        out |= found.astype(np.uint8) << np.uint8(e)
    if alive is not None:
        out[~np.asarray(alive, bool)] = 0
    return out


def degrees(masks):
    return _POP4[masks >> 4], _POP4[masks & 15]


def topology_fast(masks):
    i, o = degrees(masks)
    return np.bincount(i.astype(np.int64) * 5 + o, minlength=25).astype(np.uint64).reshape(5, 5)


def branching_fast(masks):
    i, o = degrees(masks)
    return ~((i == 1) & (o == 1))


def branching_records_fast(values, abundances, masks):
    """the 16-byte Count records {value u64, abundance u32, pad} of the branching records in flat order -> uint8[n_branching, 16]"""
    br = branching_fast(masks)
    out = np.zeros((int(br.sum()), 2), np.uint64)
    out[:, 0] = np.asarray(values, np.uint64)[br]; out[:, 1] = np.asarray(abundances, np.uint64)[br]
    return out.view(np.uint8).reshape(-1, 16)


def links_fast(values, k, masks, lookup):
    """int64[2n]: link[2i + s] = 2j + a or NONE (the rule of links_np in tests/test_unitigs_cpu.py)"""
    values = np.asarray(values, np.uint64)
    n = len(values)
    link = np.full(2 * n, NONE, np.int64)
    pal = values == revcomp_np(values, k)
    for s in (0, 1):
        nib = (masks >> (4 * s)) & 15
        i = np.flatnonzero((_POP4[nib] == 1) & ~pal)
        y = neighbour_np(values[i], k, _LOG2[nib[i]] + _U(4 * s))
        ry = revcomp_np(y, k)
        c = np.minimum(y, ry)
        found, j = lookup.find(c)
        assert found.all(), "a mask names a record that is there"
        a = np.where(c == y, 1 - s, s)
        ok = (y != ry) & (j != i) & (_POP4[(masks[j] >> (4 * a).astype(np.uint8)) & 15] == 1)
        link[2 * i[ok] + s] = 2 * j[ok] + a[ok]
    return link


LOCK_STEP_MIN = 64                                              # fewer walkers than this: a plain loop each


def paths_fast(link, alive=None):
    """unitigs as the components of the link graph -> (start record int64[n] (-1: dead), reversed bool[n], pos int64[n], n_cycles). Paths are walked from BOTH end
    records, a step at a time; the walk that began at the smaller end record is the unitig. What no walk reached lies on cycles: each walked from its smallest record,
    leaving through the right end, until it comes back."""
    n = len(link) // 2
    live = np.ones(n, bool) if alive is None else np.asarray(alive, bool)
    l0, l1 = link[0::2], link[1::2]
    ends = np.flatnonzero(live & ((l0 == NONE) | (l1 == NONE)))
    s = np.where(l0[ends] != NONE, 0, np.where(l1[ends] != NONE, 1, 0))
    terminal = np.full(len(ends), -1, np.int64)
    log_w, log_r, log_v, log_h = [], [], [], []
    act, cur, rv, h = np.arange(len(ends)), ends.copy(), s == 1, 0
    while len(act) >= LOCK_STEP_MIN:
        log_w.append(act); log_r.append(cur); log_v.append(rv); log_h.append(np.full(len(act), h, np.int64))
        t = link[2 * cur + s]
        go = t != NONE
        terminal[act[~go]] = cur[~go]
        act, t = act[go], t[go]
        cur, a = t >> 1, t & 1
        rv, s, h = a == 0, 1 - a, h + 1
    L = link.tolist()
    for w, c, ss, r in zip(act.tolist(), cur.tolist(), s.tolist(), rv.tolist()):
        rs, vs = [], []
        while True:
            rs.append(c); vs.append(r)
            t = L[2 * c + ss]
            if t == NONE:
                break
            c, a = t >> 1, t & 1
            r, ss = a == 0, 1 - a
        terminal[w] = c
        log_w.append(np.full(len(rs), w, np.int64)); log_r.append(np.array(rs, np.int64)); log_v.append(np.array(vs, bool)); log_h.append(np.arange(h, h + len(rs), dtype=np.int64))
    start = np.full(n, -1, np.int64); rev = np.zeros(n, bool); pos = np.zeros(n, np.int64)
    if log_w:
        w, r, v, hh = (np.concatenate(x) for x in (log_w, log_r, log_v, log_h))
        win = ends[w] <= terminal[w]                            # (a single record: its own terminal)
        w, r, v, hh = w[win], r[win], v[win], hh[win]
        assert len(np.unique(r)) == len(r), "every record of a path lies on one path, once"
        start[r], rev[r], pos[r] = ends[w], v, hh
        single = (l0[r] == NONE) & (l1[r] == NONE)
        assert not rev[r[single]].any()                         # a single record stands forward
    n_cycles = 0
    left = np.flatnonzero(live & (start < 0))
    if len(left):
        seen = set()
        for i in left.tolist():                                 # ascending: the first unseen record of a cycle is its smallest
            if i in seen:
                continue
            rs, vs, c, ss = [i], [False], i, 0
            while True:
                t = L[2 * c + ss]
                assert t != NONE
                j, a = t >> 1, t & 1
                if j == i:
                    break
                rs.append(j); vs.append(a == 0)
                c, ss = j, 1 - a
            assert not seen.intersection(rs) and len(set(rs)) == len(rs)
            seen.update(rs)
            rs = np.array(rs, np.int64)
            assert (start[rs] < 0).all()
            start[rs], rev[rs], pos[rs] = i, np.array(vs, bool), np.arange(len(rs))
            n_cycles += 1
    assert (start[live] >= 0).all() and (start[~live] < 0).all()
    return start, rev, pos, n_cycles


def unitigs_fast(values, abundances, k, alive=None, masks=None, lookup=None):
    """-> dict as unitigs_np of tests/test_unitigs_cpu.py gives it (without "seqs"): bases uint8[] ASCII, offsets uint64[n_unitigs + 1], kc uint64[n_unitigs], unitig
    int64[n] (-1: dead), reversed bool[n], pos int64[n], n_cycles, link, and masks, lens int64[n_unitigs], lookup"""
    values = np.asarray(values, np.uint64); ab = np.asarray(abundances, np.uint64)
    n = len(values)
    lookup = lookup or Lookup(values, alive)
    masks = masks_fast(values, k, alive, lookup) if masks is None else masks
    link = links_fast(values, k, masks, lookup)
    start, rev, pos, n_cycles = paths_fast(link, alive)
    live = start >= 0
    starts = np.unique(start[live])                             # ascending: the unitigs are numbered by start record
    unitig = np.where(live, np.searchsorted(starts, start), -1).astype(np.int64)
    nu = len(starts)
    lens = np.bincount(unitig[live], minlength=nu).astype(np.int64)
    offsets = np.zeros(nu + 1, np.uint64)
    offsets[1:] = np.cumsum(lens + (k - 1)).astype(np.uint64)
    kc = np.zeros(nu, np.uint64)
    np.add.at(kc, unitig[live], ab[live])
    # every (unitig, position) is taken once, and consecutive records overlap by k - 1 bases
    r = np.flatnonzero(live)
    first_rec = np.zeros(nu + 1, np.int64); first_rec[1:] = np.cumsum(lens)
    key = first_rec[unitig[r]] + pos[r]
    assert (pos[r] < lens[unitig[r]]).all() and (np.bincount(key, minlength=len(r)) == 1).all()
    w = np.where(rev[r], revcomp_np(values[r], k), values[r])   # the record as it stands in its unitig
    in_order = np.empty(len(r), np.int64); in_order[key] = np.arange(len(r))
    W, Un = w[in_order], unitig[r][in_order]
    same = Un[1:] == Un[:-1]
    assert ((W[:-1] & _U((1 << (2 * (k - 1))) - 1)) == (W[1:] >> _U(2)))[same].all(), "consecutive records overlap by k - 1 bases"
    # the sequence: the first base of every record at its position, and behind the last record the rest of it
    bases = np.zeros(int(offsets[-1]), np.uint8)
    at = offsets[:-1].astype(np.int64)[unitig[r]] + pos[r]
    bases[at] = LETTERS[((w >> _U(2 * (k - 1))) & _U(3)).astype(np.int64)]
    last = pos[r] == lens[unitig[r]] - 1
    for t in range(1, k):
        bases[at[last] + t] = LETTERS[((w[last] >> _U(2 * (k - 1 - t))) & _U(3)).astype(np.int64)]
    return dict(bases=bases, offsets=offsets, kc=kc, unitig=unitig, reversed=rev, pos=pos, n_cycles=n_cycles, link=link, masks=masks, lens=lens, lookup=lookup)


def unitig_links_fast(values, k, u):
    """the unitig-link CSR of the definition (unitig_links_np of tests/test_unitig_links_cpu.py) -> (offsets uint64[2 n_unitigs + 1], links uint64[n_links]): slot
    2u + side holds, ascending, v << 1 | (0: one arrives at the begin of v, 1: at its end)"""
    values = np.asarray(values, np.uint64)
    unitig, rev, pos, lens, masks, lookup = u["unitig"], u["reversed"], u["pos"], u["lens"], u["masks"], u["lookup"]
    live = unitig >= 0
    slots, entries = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for side in (0, 1):
        i = np.flatnonzero(live & (pos == (lens[np.maximum(unitig, 0)] - 1 if side == 0 else 0)))
        s = np.where(rev[i], 1 - side, side)                    # the end of the record that is this side of its unitig
        nib = (masks[i] >> (4 * s).astype(np.uint8)) & 15
        for nt in range(4):
            has = ((nib >> nt) & 1) == 1
            ii, ss = i[has], s[has]
            y = neighbour_np(values[ii], k, (nt + 4 * ss).astype(np.uint64))
            ry = revcomp_np(y, k)
            found, j = lookup.find(np.minimum(y, ry))
            assert found.all()
            a = np.where(y < ry, 1 - ss, ss)
            v = unitig[j]
            begin = a == np.where(rev[j], 0, 1)
            assert (pos[j] == np.where(begin, 0, lens[v] - 1)).all(), "one arrives at an extremity of the neighbour's unitig"
            slots.append(2 * unitig[ii] + side); entries.append((v << 1) | np.where(begin, 0, 1))
    slot, entry = np.concatenate(slots), np.concatenate(entries)
    o = np.lexsort((entry, slot))
    offs = np.zeros(2 * len(lens) + 1, np.uint64)
    offs[1:] = np.cumsum(np.bincount(slot, minlength=2 * len(lens))).astype(np.uint64)
    return offs, entry[o].astype(np.uint64)


def graph_fast(values, abundances, k, alive=None):
    """everything at once -> the dict of unitigs_fast plus link_offsets, links, topology, branching (the 16-byte records)"""
    u = unitigs_fast(values, abundances, k, alive)
    u["link_offsets"], u["links"] = unitig_links_fast(values, k, u)
    u["topology"] = topology_fast(u["masks"] if alive is None else u["masks"][np.asarray(alive, bool)])
    u["branching"] = branching_records_fast(values, abundances, u["masks"]) if alive is None else None
    return u


def records_of_counter(c):
    """the records a Counter holds, in flat (dataset) order, read as arrays -> (values uint64[n], hi uint64[n], abundances int64[n], sizes per dataset)"""
    lo, hi, ab, sizes = [], [], [], []
    for ps in range(c.nb_passes):
        for pt in range(c.nb_partitions):
            a, b, x = c.partition(ps, pt)
            lo.append(a); hi.append(b); ab.append(x.astype(np.int64)); sizes.append(len(a))
    return np.concatenate(lo), np.concatenate(hi), np.concatenate(ab), sizes


# ------------------------------------------------------------------------------------------------ reads as arrays of codes
def windows(codes, k):
    """codes uint8[R, T] -> uint64[R, T - k + 1]: the k-mer (k <= 32) at every position of every row, by doubling"""
    c = codes.astype(np.uint64)
    T = c.shape[1]
    assert 1 <= k <= 32 and T >= k
    pw, w = {1: c}, 1
    while 2 * w <= k:
        v = pw[w]
        pw[2 * w] = (v[:, : v.shape[1] - w] << _U(2 * w)) | v[:, w:]
        w *= 2
    out, width = None, 0
    for w in sorted(pw, reverse=True):
        if not k & w:
            continue
        if out is None:
            out, width = pw[w], w
        else:
            m = T - (width + w) + 1
            out = (out[:, :m] << _U(2 * w)) | pw[w][:, width: width + m]
            width += w
    return out


def canonical_windows(codes, k):
    x = windows(codes, k).reshape(-1)
    return np.minimum(x, revcomp_np(x, k))


def pack_groups(groups):
    """-> (bases uint8[] ASCII, offsets uint64[n_reads + 1]) as Counter.count takes them"""
    rows, lens = [], []
    for g, copies in groups:
        for _ in range(copies):
            rows.append(LETTERS[g].reshape(-1)); lens.append(np.full(g.shape[0], g.shape[1], np.uint64))
    offs = np.zeros(sum(len(x) for x in lens) + 1, np.uint64)
    offs[1:] = np.cumsum(np.concatenate(lens))
    return np.concatenate(rows), offs


def reads_of_groups(groups):
    """the same reads as strings, in the same order"""
    return [LETTERS[row].tobytes().decode() for g, copies in groups for _ in range(copies) for row in g]


class Built:
    """a constructed input. groups: [(codes uint8[R, T], copies)]: R reads of T bases, each given ``copies`` times. n: its distinct canonical k-mers (= records),
    n_unitigs: its unitigs, dies: {"tips" / "bulges" / "ec": the canonical k-mers that kind removes}, counts: the structures it holds"""

    def __init__(self, k, groups, n_unitigs, shared, dies=None, counts=None, circular=()):
        self.k, self.groups, self.n_unitigs, self.dies, self.counts = k, groups, n_unitigs, dies or {}, counts or {}
        kmers = np.concatenate([canonical_windows(g, k) for g, _ in groups])
        self.n = len(kmers)
        self.kmers = kmers
        # exact n: every k-mer position is another canonical k-mer; every (k-1)-mer position another canonical (k-1)-mer, but for the ``shared`` ones the shapes are
        # made of (and the one a circular read repeats at its end); no (k-1)-mer is its own reverse complement (it would be a neighbour of itself)
        ok = len(np.unique(kmers)) == self.n
        sub = np.concatenate([windows(g, k - 1).reshape(-1) for g, _ in groups])
        rsub = revcomp_np(sub, k - 1)
        ok = ok and len(np.unique(np.minimum(sub, rsub))) == len(sub) - shared - len(circular) and not (sub == rsub).any()
        self.ok = bool(ok)

    def pack(self):
        return pack_groups(self.groups)

    def reads(self):
        return reads_of_groups(self.groups)

    def alive_after(self, values, kinds):
        """bool[n]: the records left once the k-mers of ``kinds`` have died"""
        dead = np.concatenate([self.dies[kd] for kd in kinds] + [np.zeros(0, np.uint64)])
        return ~np.isin(np.asarray(values, np.uint64), dead)


def first_good(make, seed, tries=16):
    """the first of make(seed), make(seed + 1), ... whose k-mers and (k-1)-mers are distinct as it means them"""
    for s in range(seed, seed + tries):
        b = make(np.random.default_rng(s))
        if b.ok:
            return b
    raise AssertionError("no input with distinct k-mers found in %d seeds" % tries)


def rand(rng, rows, cols):
    return rng.integers(0, 4, (rows, cols), dtype=np.uint8)


def other_than(rng, a):
    """a code that differs from a, per element"""
    return ((a + 1 + rng.integers(0, 3, a.shape, dtype=np.uint8)) & 3).astype(np.uint8)


def path_groups(rng, lengths, k):
    """random reads of L + k - 1 bases per L of ``lengths`` (record counts), grouped by length"""
    ls, cnt = np.unique(np.asarray(lengths, np.int64), return_counts=True)
    return [(rand(rng, int(c), int(L) + k - 1), 1) for L, c in zip(ls, cnt)]


def lengths_for(n, n_paths=None, choices=(1, 2, 3)):
    """record counts of isolated paths with the exact total n. n_paths None: 1, 2, 3, 1, 2, 3, ... with the last ones cut to fit; else that many paths of 1 or 2 records"""
    if n_paths is not None:
        assert n_paths <= n <= 2 * n_paths
        return [2] * (n - n_paths) + [1] * (2 * n_paths - n)
    per = sum(choices)
    lens = list(choices) * (n // per)
    lens += [1] * (n - sum(lens))
    assert sum(lens) == n
    return lens


def isolated_paths(lengths, k=31, seed=0):
    """isolated paths of the given record counts: n = sum(lengths), one unitig each"""
    return first_good(lambda rng: Built(k, path_groups(rng, lengths, k), len(lengths), 0), seed)


def long_path(n_records, k=31, seed=0):
    return isolated_paths([n_records], k, seed)


def circle_groups(rng, L, k, codes=(0, 1, 2, 3)):
    seq = np.array(codes, np.uint8)[rng.integers(0, len(codes), (1, L))]
    return [(np.concatenate([seq, seq[:, : k - 1]], 1), 1)]       # circle_read: every k-mer of the circle once


def circles_and_paths(circle_lengths, path_lengths, k=31, seed=0, high_circles=()):
    """random circular sequences (each one read, one cyclic unitig) and isolated paths. high_circles: lengths of circles over C and G alone: every k-mer of such a
    circle and its reverse complement begin with C or G, so its canonical value is at least 4^k / 4, which 7 / 16 of all canonical k-mers lie below: in one dataset
    its records stand behind the first 7 / 16 of random records (Built.high: those k-mers)"""
    def make(rng):
        groups = [g for L in circle_lengths for g in circle_groups(rng, L, k)]
        high = [g for L in high_circles for g in circle_groups(rng, L, k, (1, 3))]
        n_c = len(circle_lengths) + len(high_circles)
        b = Built(k, groups + high + path_groups(rng, path_lengths, k), n_c + len(path_lengths), 0, circular=[0] * n_c, counts=dict(circles=n_c))
        b.high = np.concatenate([canonical_windows(g, k) for g, _ in high] + [np.zeros(0, np.uint64)])
        return b
    return first_good(make, seed)


ARM = 2                                                         # records per arm of the tips, bubbles and connectors: k + 1 bases, one too long for a tip at max_len_topo = k
BUBBLE_COV, EC_COV = 3, 5


def padding_plus_structures(pad_lengths, k=31, seed=0, forks=0, tips=0, bubbles=0, ecs=0):
    """isolated paths (``pad_lengths``: record counts) and, scattered among them by their random values, branching structures:
    forks   : three arms of three records on one junction (forks_and_paths of tests/test_gpu_tips.py): 9 records, 3 unitigs; they stay at max_len_topo = k
    tips    : a path of 2 ARM records and a one-record branch off its middle: 2 ARM + 1 records, 3 unitigs; the branch is a tip of k bases, then the path is one unitig
    bubbles : ARM records, an SNP, ARM records, read BUBBLE_COV times, and the other allele once: 2 ARM + 2 k records, 4 unitigs; the allele read once is a bulge
    ecs     : two paths of 2 ARM records read EC_COV times and a connector of k records, read once, from the middle of one to the middle of the other (the Z of
              tests/golden/reference_simplify_vectors.json): 4 ARM + k records, 5 unitigs; the connector is an erroneous connection
    -> Built with dies = the k-mers of the branch / other-allele / connector reads"""
    def make(rng):
        groups, dies = path_groups(rng, pad_lengths, k), {}
        if forks:
            lead = rand(rng, forks, k - 1)
            groups += [(np.hstack([lead, np.full((forks, 1), c, np.uint8), rand(rng, forks, 2)]), 1) for c in (0, 1)] + [(np.hstack([rand(rng, forks, 3), lead]), 1)]
        main = rand(rng, tips, 2 * ARM + k - 1)
        branch = np.hstack([main[:, ARM: ARM + k - 1], other_than(rng, main[:, ARM + k - 1: ARM + k])])
        S = rand(rng, bubbles, 2 * ARM + 2 * k - 1)
        c = ARM + k - 1
        allele = np.hstack([S[:, c - (k - 1): c], other_than(rng, S[:, c: c + 1]), S[:, c + 1: c + k]])
        M1, M2 = rand(rng, ecs, 2 * ARM + k - 1), rand(rng, ecs, 2 * ARM + k - 1)
        a, b = M1[:, c], M2[:, ARM - 1]
        inner = np.zeros(ecs, np.uint8)
        for code in (3, 2, 1, 0):                               # a base that continues neither M1 nor, read backwards, M2
            inner[(a != code) & (b != code)] = code
        conn = np.hstack([M1[:, c - (k - 1): c], inner[:, None], M2[:, ARM: ARM + k - 1]])
        for n_, gs in ((tips, [(main, 1), (branch, 1)]), (bubbles, [(S, BUBBLE_COV), (allele, 1)]), (ecs, [(M1, EC_COV), (M2, EC_COV), (conn, 1)])):
            if n_:
                groups += gs
        dies = dict(tips=canonical_windows(branch, k) if tips else np.zeros(0, np.uint64), bulges=canonical_windows(allele, k) if bubbles else np.zeros(0, np.uint64),
                    ec=canonical_windows(conn, k) if ecs else np.zeros(0, np.uint64))
        return Built(k, groups, len(pad_lengths) + 3 * forks + 3 * tips + 4 * bubbles + 5 * ecs, 2 * forks + tips + 2 * bubbles + 2 * ecs, dies,
                     dict(forks=forks, tips=tips, bubbles=bubbles, ecs=ecs))
    return first_good(make, seed)


def structure_records(k, forks=0, tips=0, bubbles=0, ecs=0):
    return 9 * forks + (2 * ARM + 1) * tips + (2 * ARM + 2 * k) * bubbles + (4 * ARM + k) * ecs


def expected_simplify_log(b, values, abundances, p, cache=None):
    """the log simplify_np of tests/test_simplify_cpu.py would give for a Built whose kinds die as the construction means them: each kind's k-mers in the first round
    that kind runs, nothing afterwards. p: the parameters (tip_rounds, bulge_rounds, ec_rounds, max_sweeps). The number of unitigs at every round comes from the fast
    statement over the records alive then (``cache``: a dict that keeps them between calls over the same records). -> (log, alive bool[n])"""
    values = np.asarray(values, np.uint64)
    alive = np.ones(len(values), bool)
    cache, log = {} if cache is None else cache, []
    rounds = dict(tips=p["tip_rounds"], bulges=p["bulge_rounds"], ec=p["ec_rounds"])

    def n_unitigs():
        key = alive.tobytes()
        if key not in cache:
            cache[key] = len(unitigs_fast(values, abundances, b.k, alive)["lens"])
        return cache[key]

    def phase(kind, sweep):
        gone = 0
        for _ in range(rounds[kind]):
            dead = alive & np.isin(values, b.dies[kind])
            hits = {"tips": b.counts["tips"], "bulges": b.counts["bubbles"], "ec": b.counts["ecs"]}[kind] if dead.any() else 0
            log.append((kind, sweep, n_unitigs(), hits, int(dead.sum())))
            alive[dead] = False
            gone += int(dead.sum())
            if not hits:
                break
        return gone

    phase("tips", 0)
    for sweep in range(1, p["max_sweeps"] + 1):
        if not phase("bulges", sweep) + phase("ec", sweep) + phase("tips", sweep):
            break
    return log, alive


# ------------------------------------------------------------------------------------------------ wide keys: isolated paths at k = 33, in closed form
def wide_isolated_paths(lengths, seed=0):
    """isolated paths at k = 33 (two words per k-mer) for ONE dataset, whose records are the sorted canonical k-mers, with everything the device returns in closed form:
    a read is one unitig that starts at whichever end record has the smaller index; its bases are the read, or the read's reverse complement; the unitigs are numbered by
    start record -> (bases, offsets of the reads, expected dict: lo, hi, masks, bases, offsets, kc, unitig, reversed, pos, n)"""
    k = 33
    for s in range(seed, seed + 16):
        rng = np.random.default_rng(s)
        per = []                                                # per length class: the reads, their reverse complements, the two words of every k-mer on either strand
        groups = path_groups(rng, lengths, k)
        sub, rid0 = [], 0
        for g, _ in groups:
            R, T = g.shape
            L = T - k + 1
            rc = (g[:, ::-1] ^ 2).astype(np.uint8)
            lo_f, lo_r = windows(g[:, 1:], 32), windows(rc[:, 1:], 32)[:, ::-1]      # window w of the read is window L - 1 - w of its reverse complement
            hi_f, hi_r = g[:, :L].astype(np.uint64), rc[:, :L][:, ::-1].astype(np.uint64)
            sub.append(windows(g, 32).reshape(-1))
            per.append((g, rc, lo_f, hi_f, lo_r, hi_r, rid0))
            rid0 += R
        sub = np.concatenate(sub); rsub = revcomp_np(sub, 32)
        if len(np.unique(np.minimum(sub, rsub))) != len(sub) or (sub == rsub).any():
            continue
        lo, hi, fwd, rid, win, rlen, before, after = ([] for _ in range(8))
        for g, rc, lo_f, hi_f, lo_r, hi_r, r0 in per:
            R, L = lo_f.shape
            f = (hi_f < hi_r) | ((hi_f == hi_r) & (lo_f < lo_r))  # the read's strand is the canonical one (k odd: never equal)
            lo.append(np.where(f, lo_f, lo_r).reshape(-1)); hi.append(np.where(f, hi_f, hi_r).reshape(-1)); fwd.append(f.reshape(-1))
            rid.append(np.repeat(np.arange(r0, r0 + R), L)); win.append(np.tile(np.arange(L), R)); rlen.append(np.full(R * L, L))
            pad = np.full((R, 1), 255, np.uint8)
            before.append(np.hstack([pad, g[:, : L - 1]]).reshape(-1)); after.append(np.hstack([g[:, k: k + L - 1], pad]).reshape(-1))
        lo, hi, fwd, rid, win, rlen, before, after = (np.concatenate(x) for x in (lo, hi, fwd, rid, win, rlen, before, after))
        o = np.lexsort((lo, hi))
        if len(o) > 1 and ((lo[o][1:] == lo[o][:-1]) & (hi[o][1:] == hi[o][:-1])).any():
            continue
        lo, hi, fwd, rid, win, rlen, before, after = (x[o] for x in (lo, hi, fwd, rid, win, rlen, before, after))
        n, n_reads = len(lo), rid0
        idx = np.arange(n)
        # masks: the base after the window extends the read's strand to the right, the base before it to the left; on the other strand right and left swap and the
        # base is complemented
        masks = np.zeros(n, np.uint8)
        has = after != 255
        masks[has] |= np.where(fwd[has], 1 << after[has], 16 << (after[has] ^ 2)).astype(np.uint8)
        has = before != 255
        masks[has] |= np.where(fwd[has], 16 << before[has], 1 << (before[has] ^ 2)).astype(np.uint8)
        # placement: the end records of read r are its windows 0 and L - 1
        first = np.full(n_reads, -1, np.int64); last = np.full(n_reads, -1, np.int64)
        first[rid[win == 0]] = idx[win == 0]; last[rid[win == rlen - 1]] = idx[win == rlen - 1]
        single = first == last
        as_read = np.where(single, fwd[first], first < last)    # the unitig spells the read (else its reverse complement); a single record stands forward
        start = np.minimum(first, last)
        rank = np.empty(n_reads, np.int64); rank[np.argsort(start)] = np.arange(n_reads)
        unitig = rank[rid]
        pos = np.where(as_read[rid], win, rlen - 1 - win)
        rev = fwd != as_read[rid]
        L_of = np.zeros(n_reads, np.int64); L_of[rid[win == 0]] = rlen[win == 0]
        offsets = np.zeros(n_reads + 1, np.uint64)
        by_rank = np.argsort(rank)
        offsets[1:] = np.cumsum(L_of[by_rank] + k - 1).astype(np.uint64)
        out = np.zeros(int(offsets[-1]), np.uint8)
        r0 = 0
        for g, rc, *_ in per:
            R, T = g.shape
            ids = np.arange(r0, r0 + R)
            text = LETTERS[np.where(as_read[ids][:, None], g, rc)]
            out[(offsets[:-1].astype(np.int64)[rank[ids]][:, None] + np.arange(T)[None, :]).reshape(-1)] = text.reshape(-1)
            r0 += R
        bases, offs = pack_groups(groups)
        exp = dict(lo=lo, hi=hi, masks=masks, bases=out, offsets=offsets, kc=L_of[by_rank].astype(np.uint64), unitig=unitig, reversed=rev, pos=pos, n=n, reads=reads_of_groups(groups))
        return bases, offs, exp
    raise AssertionError("no k = 33 input with distinct k-mers found")
