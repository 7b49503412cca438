"""Token sets for the embedding kernels (csrc/embedding.hip: embed_fwd_*, embed_hist / _block_prefix / _scan / _fill / _gather /
_gather_finish behind uic_embedding_*), the launch geometry of those kernels restated, a classifier that says which branches of
that geometry a token set reaches, and a plain numpy restatement of the bucketed sum -- shared by tests/test_embedding_cases_host.py
(the cases reach every class; the restatement equals index_add_) and tests/test_gpu_embedding.py (the kernels themselves).

Rows are time-major: row i = t * N + n carries tokens[n, t].  A case is built from its `rows`, the tokens in row order, so a builder
decides bucket sizes (how often a token occurs) and a seeded permutation scatters the occurrences over the positions; the sorted
list of the kernels then holds the buckets back to back in token order, at offsets the builder chose.
"""
import functools

import numpy as np

# ---- the launch geometry of the embedding kernels, restated (tests/test_gpu_embedding.py holds SCRATCH against the library) ----
HIST_BLK = 1024          # positions per histogram / fill workgroup (EMB_BLK)
SCAN_TRIP = 4096         # keys per trip of the single-workgroup scan: 1024 threads, 4 keys each
SCAN_PER_THREAD = 4
CH = 16                  # list entries per gather workgroup (EMB_CH)
FG = 8                   # groups of 128 threads that share a straddling bucket's partial rows in the finish kernel (EMB_FG)
FINISH_COLS = 128        # float4 columns per trip of the finish kernel (and of the gather kernel: 128 threads)
FWD_ROWS_PER_WG = 4      # the bf16 row kernel: one wave per row, 4 waves
FWD_GRID_CAP = 8192      # ... and at most this many workgroups
FWD_LANE_ELEMS = 8       # ... 8 elements per lane and trip
LANES = 64
INT64_MIN = -2 ** 63


def _up64(x):
    return (x + 63) // 64 * 64


def hist_blocks(positions):
    return -(-positions // HIST_BLK)


def chunk_slots(N, T):
    """Partial-row slots per plane: every half of a split list is rounded up to whole workgroups."""
    return N * T // CH + 2


def scratch_ints(N, T, V1, E):
    """cnt | off | (unused), 2 V1 + 1 ints each, | perm [N T] (+ 64, rounded to 64) | cntb [blocks, 2 V1] (rounded to 64) | part [2, slots, E]."""
    return _up64(3 * (2 * V1 + 1) + N * T + 64) + _up64(hist_blocks(N * T) * 2 * V1) + 2 * chunk_slots(N, T) * E


def fwd_row_kernel_trips(rows, E):
    """(trips of a workgroup over the rows, trips of a lane over a row) of the bf16 row kernel."""
    wgs = min(FWD_GRID_CAP, -(-rows // FWD_ROWS_PER_WG))
    return -(-rows // (wgs * FWD_ROWS_PER_WG)), -(-(E // FWD_LANE_ELEMS) // LANES)


# ---- cases ----
class Case:
    """One token set and how the backward pass is asked to treat it.  Nothing here is modified after construction."""

    def __init__(self, name, N, T, V1, E, rows, ld=None, split=0, skip=-1, drop_p=0.0, xt="none"):
        rows = np.asarray(rows, dtype=np.int64)
        assert rows.shape == (N * T,), (name, rows.shape, N, T)
        self.name, self.N, self.T, self.V1, self.E = name, N, T, V1, E
        self.ld = T if ld is None else ld
        self.split, self.skip, self.drop_p, self.xt = split, skip, drop_p, xt
        assert self.ld >= T and 0 <= split < max(T, 1) and skip < V1 and E % 4 == 0
        self.rows = rows
        tok = (np.arange(N)[:, None] * 7 + np.arange(self.ld)[None, :] * 3 + 1) % V1          # the columns behind T: other tokens
        tok = tok.astype(np.int64)
        tok[:, :T] = rows.reshape(T, N).T
        self.tokens = np.ascontiguousarray(tok)
        self.seed = sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)

    @property
    def positions(self):
        return self.N * self.T

    @property
    def inv_keep(self):
        return 1.0 / (1.0 - self.drop_p)

    def row_token(self):
        """The table row of every position: tokens outside [0, V1) count as token 0."""
        r = self.rows
        return np.where((r < 0) | (r >= self.V1), 0, r)

    def keys(self):
        k = self.row_token().copy()
        if self.split:
            k[self.split * self.N:] += self.V1
        return k

    def nkeys(self):
        return (2 if self.split else 1) * self.V1

    def halves(self):
        """(half, base, total, keybase, chunk0) of every gather launch."""
        if not self.split:
            return [(0, 0, self.positions, 0, 0)]
        s = self.split * self.N
        return [(0, 0, s, 0, 0), (1, s, self.positions, self.V1, -(-s // CH))]

    def grad(self):
        """Integers in [-8, 8]: with inv_keep 1, 2 or 4 every partial sum is an integer below 2^24, exact in f32 in any order."""
        return np.random.default_rng(self.seed).integers(-8, 9, size=(self.positions, self.E)).astype(np.float32)

    def __repr__(self):
        return "Case(%s)" % self.name


def scatter(sizes, seed):
    """[(token, count), ...] -> the tokens in a seeded random row order."""
    r = np.concatenate([np.full(c, t, dtype=np.int64) for t, c in sizes]) if sizes else np.zeros(0, dtype=np.int64)
    return np.random.default_rng(seed).permutation(r)


def layout_a(tail):
    """Bucket sizes 1, 2, 13, 16 (aligned), 8, 16 (from the middle of a workgroup), 17, 7, 129, 145, 160, 30 and `tail`, at list offsets
    0 1 3 16 32 40 56 73 80 209 354 514 544: classes (a) to (g) of classify().  Token 13 never occurs."""
    return [(0, 1), (1, 2), (2, 13), (3, 16), (4, 8), (5, 16), (6, 17), (7, 7), (8, 129), (9, 145), (10, 160), (11, 30)] + ([(12, tail)] if tail else [])


LAYOUT_A_V1 = 14
LAYOUT_B = [(0, 40), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (8, 52)]      # 97 entries: keys 0 and V1 - 1 straddle, the last workgroup holds 1
LAYOUT_B_V1 = 9


def geometric_rows(n, V1, seed, p=0.08):
    return np.minimum(np.random.default_rng(seed).geometric(p, size=n) - 1, V1 - 1).astype(np.int64)


def zipf_rows(N, T, words, seed):
    """Captions of Zipf(1) words 1...words-1, token 0 behind each caption's end; row order (time-major)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, words)
    w = rng.choice(np.arange(1, words), size=(N, T), p=p / p.sum())
    length = rng.integers(T // 2, T + 1, size=N)
    w[np.arange(T)[None, :] >= length[:, None]] = 0
    return w.T.reshape(-1).astype(np.int64)


XT_MODES = ("none", "fwd_f32", "fwd_bf16", "hand_f32", "hand_bf16")
DROPS = (0.0, 0.5, 0.75)


def _variant(i):
    """A (drop_p, xt) pair per case, all fifteen in turn."""
    return dict(drop_p=DROPS[i % 3], xt=XT_MODES[(i // 3 + i) % 5])


@functools.lru_cache(maxsize=None)
def backward_cases():
    cs = []

    def add(name, N, T, V1, E, rows, **kw):
        v = _variant(len(cs))
        v.update(kw)
        cs.append(Case(name, N, T, V1, E, rows, **v))

    # N T = 1 ... 2049: 1, 1, 2 and 3 histogram blocks; T = 1 with ld_tokens = 1 is the pivot NMT calling shape
    for N, T in ((1, 1), (5, 3), (4, 4), (17, 1), (33, 31), (64, 16), (41, 25), (683, 3)):
        add("size%d" % (N * T), N, T, 37, 8, geometric_rows(N * T, 37, N * T), ld=T if T == 1 else T + 2)
    # one bucket over the whole list
    for N, T in ((16, 1), (10, 16), (7, 23), (683, 3)):
        add("onetoken%d" % (N * T), N, T, 5, 8, np.full(N * T, 3, dtype=np.int64))
    # constructed bucket sizes, under every (drop_p, xt) and every kind of skip_token
    for i in range(15):
        add("layoutA-%d" % i, 61, 9, LAYOUT_A_V1, 8, scatter(layout_a(5), 100 + i), ld=11, **_variant(i))
    for skip, what in ((0, "cold0"), (4, "cold"), (10, "hot"), (13, "absent"), (11, "hotlast")):
        add("layoutA-skip-%s" % what, 61, 9, LAYOUT_A_V1, 8, scatter(layout_a(5), 7), skip=skip)
    for E in (4, 8, 12, 512, 516):               # one lane; 8; 12; exactly one trip of the finish kernel; a second trip with one lane
        add("layoutB-E%d" % E, 97, 1, LAYOUT_B_V1, E, scatter(LAYOUT_B, E), ld=1)
        add("layoutA-E%d" % E, 61, 9, LAYOUT_A_V1, E, scatter(layout_a(5), E))
    for skip in (0, 8):                          # the straddling bucket is key 0 / key V1 - 1, and it is the padding index
        add("layoutB-skip%d" % skip, 97, 1, LAYOUT_B_V1, 8, scatter(LAYOUT_B, skip), skip=skip)
    # one Zipf(1) draw: ~300 words over 2304 positions, ld_tokens > T
    add("zipf", 128, 18, 300, 516, zipf_rows(128, 18, 300, 5), ld=20, drop_p=0.5, xt="fwd_bf16")
    add("zipf-skip0", 128, 18, 300, 8, zipf_rows(128, 18, 300, 6), ld=20, skip=0)
    # key counts around the scan's 4096-key trips; the hot tokens sit at 0 and at V1 - 1
    for V1 in (1, 3, 4, 5, 4095, 4096, 4097, 8193):
        rng = np.random.default_rng(V1)
        rows = np.concatenate([np.zeros(17, dtype=np.int64), np.full(18, V1 - 1, dtype=np.int64), rng.integers(0, V1, size=13)])
        add("keys%d" % V1, 6, 8, V1, 8, rng.permutation(rows))
    for V1 in (2049, 4097):                      # 4098 and 8194 keys with a split
        rng = np.random.default_rng(V1 + 1)
        rows = np.concatenate([rng.permutation(np.concatenate([np.zeros(a, dtype=np.int64), np.full(b, V1 - 1, dtype=np.int64), rng.integers(0, V1, size=c)]))
                               for a, b, c in ((7, 9, 2), (12, 14, 4))])
        add("keys%d-split" % V1, 6, 8, V1, 8, rows, split=3)
    # tokens outside the table among ordinary ones: all of them count as token 0
    rng = np.random.default_rng(11)
    rows = np.array([-1] * 6 + [21] * 6 + [2 ** 40] * 5 + [INT64_MIN] * 5 + [2 ** 31] * 3 + [0] * 2 + rng.integers(1, 21, size=21).tolist(), dtype=np.int64)
    add("outside", 8, 6, 21, 8, rng.permutation(rows), ld=9)
    add("outside-skip0", 8, 6, 21, 8, rng.permutation(rows), ld=9, skip=0)
    # the two-half mode: split = 1, T - 1 and a middle value; split * N a multiple of 16 and not; layout A in half 1 and in half 0
    small = [(0, 20), (3, 1), (5, 3), (9, 30), (12, 7)]                                        # 61 entries
    mid = [(0, 200), (1, 3), (2, 1), (8, 50), (10, 17), (11, 16), (12, 33)]                     # 320 entries
    for i in range(3):
        add("split1-%d" % i, 61, 10, LAYOUT_A_V1, 8, np.concatenate([scatter(small, 20 + i), scatter(layout_a(5), 30 + i)]), split=1, ld=12)
        add("splitlast-%d" % i, 61, 10, LAYOUT_A_V1, 8, np.concatenate([scatter(layout_a(5), 40 + i), scatter(small, 50 + i)]), split=9)
        add("splitmid-%d" % i, 64, 14, LAYOUT_A_V1, 8, np.concatenate([scatter(mid, 60 + i), scatter(layout_a(32), 70 + i)]), split=5)
    add("split1-skiphot", 61, 10, LAYOUT_A_V1, 8, np.concatenate([scatter(small, 24), scatter(layout_a(5), 34)]), split=1, skip=10)
    add("splitmid-E516", 64, 14, LAYOUT_A_V1, 516, np.concatenate([scatter(mid, 64), scatter(layout_a(32), 74)]), split=5)
    add("zipf-split", 128, 18, 300, 12, zipf_rows(128, 18, 300, 8), ld=20, split=7)
    add("size2049-split", 683, 3, 37, 8, geometric_rows(2049, 37, 9), split=2)
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def case_by_name(name):
    return next(c for c in backward_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def dirty_case():
    """Larger than every case in positions, table rows and row width: what runs between two runs of a case to leave stale (but
    in-range) entries in every region of the scratch."""
    c = Case("dirty", 128, 19, 8200, 520, zipf_rows(128, 19, 8200, 99), ld=21)
    for b in backward_cases():
        assert c.positions > b.positions and c.V1 > b.V1 and c.E > b.E
    return c


# ---- which branches of the geometry a case reaches ----
CLASSES = ("a", "b", "c", "d", "e_inside", "e_arriving", "f", "g", "h_key0", "h_keylast", "i_short", "i_one", "j", "k",
           "l_aligned", "l_unaligned", "l_b", "l_c", "l_d", "m")


def sorted_list(case):
    """(perm, off): the stable sort of the positions by key and the exclusive prefix of the key counts (off[nkeys] = positions)."""
    keys = case.keys()
    perm = np.argsort(keys, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=case.nkeys()))])
    return perm, off


def classify(case):
    """The classes of CLASSES the case reaches (see the comments)."""
    hit = set()
    keys = case.keys()
    perm, off = sorted_list(case)
    tok_sorted = case.row_token()[perm]
    for half, base, total, keybase, _ in case.halves():
        gw = -(-(total - base) // CH)
        first_run_from_earlier = np.zeros(gw, dtype=bool)
        last_run_goes_on = np.zeros(gw, dtype=bool)
        owner_of_first, owner_of_last = np.full(gw, -1), np.full(gw, -2)
        for key in range(keybase, keybase + case.V1):
            b0, b1 = off[key], off[key + 1]
            if b0 == b1:
                continue
            w0, w1 = (b0 - base) // CH, (b1 - 1 - base) // CH
            straddle = w1 > w0
            if not straddle and (b0 - base) % CH != 0:
                hit.add("a")                                  # wholly inside one workgroup, not its first run
            if (b1 - base) % CH == 0 and b1 < total:
                hit.add("e_arriving" if straddle else "e_inside")     # ends at a workgroup's last entry, another workgroup follows
            if not straddle:
                continue
            tok = key - keybase
            cls = []
            if w1 - w0 == 1:
                cls.append("b")                               # exactly two workgroups
            if w1 - w0 >= FG + 2:
                cls.append("c")                               # >= 10 partial rows: every finish group has one, some have two
            if (b0 - base) % CH == 0:
                cls.append("d")                               # begins at a workgroup's first entry
            hit.update(cls)
            if half == 1:
                hit.update("l_" + x for x in cls)
            if tok == 0:
                hit.add("h_key0")
            if tok == case.V1 - 1:
                hit.add("h_keylast")
            if tok == case.skip:
                hit.add("m")
            if w1 - w0 >= 2:
                hit.add("g")                                  # a middle workgroup filled by this bucket
            first_run_from_earlier[w0 + 1:w1 + 1] = True
            owner_of_first[w0 + 1:w1 + 1] = key
            last_run_goes_on[w0:w1] = True
            owner_of_last[w0:w1] = key
        if (first_run_from_earlier & last_run_goes_on & (owner_of_first != owner_of_last)).any():
            hit.add("f")                                      # both planes of one chunk are written
        last = total - base - (gw - 1) * CH
        if last < CH:
            hit.add("i_short")
        if last == 1:
            hit.add("i_one")
        if case.split:
            hit.add("l_aligned" if (case.split * case.N) % CH == 0 else "l_unaligned")
    nblk = hist_blocks(case.positions)
    if nblk > 1:
        blocks_of = {}
        for b in range(nblk):
            for k in np.unique(keys[b * HIST_BLK:(b + 1) * HIST_BLK]):
                blocks_of[k] = blocks_of.get(k, 0) + 1
        if max(blocks_of.values()) >= 3:
            hit.add("j")                                      # the prefix over the blocks adds up two earlier blocks
    for w in range(0, case.positions, LANES):                 # a wave of the histogram kernel: two aggregation rounds, then plain atomics
        lanes = keys[w:w + LANES]
        first = lanes[0]
        rest = lanes[lanes != first]
        if rest.size:
            rest = rest[rest != rest[0]]
            if rest.size and np.unique(rest).size < rest.size:
                hit.add("k")                                  # two lanes of the fallback add to the same counter
    assert tok_sorted.size == case.positions
    return hit


# ---- the pipeline restated: list order, ownership, the two planes of partial rows, the finish order ----
def restated_sort(case):
    """histogram per block -> exclusive prefix over the blocks -> exclusive scan over the keys -> fill: perm and off as the kernels
    build them."""
    keys, nkeys, total = case.keys(), case.nkeys(), case.positions
    nblk = hist_blocks(total)
    cntb = np.zeros((nblk, nkeys), dtype=np.int64)
    for b in range(nblk):
        cntb[b] = np.bincount(keys[b * HIST_BLK:(b + 1) * HIST_BLK], minlength=nkeys)
    cnt = cntb.sum(0)
    before = np.cumsum(cntb, axis=0) - cntb
    off = np.zeros(nkeys + 1, dtype=np.int64)
    carry = 0
    for trip in range(0, nkeys, SCAN_TRIP):                   # the carried total of the scan's trips
        x = cnt[trip:trip + SCAN_TRIP]
        off[trip:trip + x.size] = carry + np.cumsum(x) - x
        carry += int(x.sum())
    off[nkeys] = carry
    perm = np.full(total, -1, dtype=np.int64)
    for b in range(nblk):
        seen = {}
        for i in range(b * HIST_BLK, min(total, (b + 1) * HIST_BLK)):
            k = int(keys[i])
            rank = seen.get(k, 0)
            seen[k] = rank + 1
            slot = off[k] + before[b, k] + rank
            assert perm[slot] == -1
            perm[slot] = i
    return perm, off


def restated_gather(case, perm, off, g, table, halves=(0, 1)):
    """embed_gather_kernel + embed_gather_finish_kernel in float64 on the masked gradients g [positions, E]; `table` is what prepare
    zeroed (or what an earlier half left) and is updated in place.  Partial-row slots start as NaN: one that is read before it is
    written poisons the result.  Returns how often each table row was stored per launch (ownership: at most once)."""
    E, tokrow, skip = case.E, case.row_token(), case.skip
    accum = case.split > 0
    part = np.full((2, chunk_slots(case.N, case.T), E), np.nan)
    stores = []
    for half, base, total, keybase, chunk0 in case.halves():
        if half not in halves or total == base:
            continue
        count = np.zeros(case.V1, dtype=np.int64)
        gw = -(-(total - base) // CH)

        def store(tok, v):
            table[tok] = v * case.inv_keep + (table[tok] if accum else 0.0)
            count[tok] += 1
        for w in range(gw):
            start = base + w * CH
            n = min(CH, total - start)
            pos = perm[start:start + n]
            tk = tokrow[pos]
            acc = np.zeros(E)
            for j in range(n):
                acc = acc + g[pos[j]]
                if j + 1 == n or tk[j + 1] != tk[j]:
                    if tk[j] != skip:
                        b0, b1 = off[keybase + tk[j]], off[keybase + tk[j] + 1]
                        if b0 >= start and b1 <= start + n:
                            store(tk[j], acc)
                        else:
                            part[1 if b0 >= start else 0, chunk0 + w] = acc
                    acc = np.zeros(E)
        for w in range(gw):
            start = base + w * CH
            n = min(CH, total - start)
            tok = tokrow[perm[start + n - 1]]
            if tok == skip:
                continue
            b0, b1 = off[keybase + tok], off[keybase + tok + 1]
            if b0 < start or b1 <= start + n:
                continue
            c_last = (b1 - 1 - base) // CH
            sums = []
            for grp in range(FG):
                acc = part[1, chunk0 + w].copy() if grp == 0 else np.zeros(E)
                for k in range(w + 1 + grp, c_last + 1, FG):
                    acc = acc + part[0, chunk0 + k]
                sums.append(acc)
            acc = sums[0]
            for grp in range(1, FG):
                acc = acc + sums[grp]
            store(tok, acc)
        stores.append(count)
    return stores


def reference(case, g, halves=(0, 1)):
    """zeros(V1, E, float64).index_add_(0, token of the row, g) * inv_keep over the rows of the given halves; the skip_token row is 0."""
    import torch
    lo = 0 if (0 in halves or not case.split) else case.split * case.N
    hi = case.positions if (1 in halves or not case.split) else case.split * case.N
    idx = torch.from_numpy(case.row_token()[lo:hi])
    ref = torch.zeros(case.V1, case.E, dtype=torch.float64).index_add_(0, idx, torch.from_numpy(np.asarray(g[lo:hi], dtype=np.float64)))
    ref *= case.inv_keep
    if case.skip >= 0:
        ref[case.skip] = 0
    return ref


# ---- the dropout hash of csrc/uic_common.h (uic_drop_scale), restated in uint32 ----
def drop_keep(n, p, seed, site, base):
    """True where element base + i (modulo 2^32) is kept at dropout probability p."""
    M = 0xFFFFFFFF
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(base % 2 ** 32)) & np.uint64(M)
    x = (idx * np.uint64(0x9E3779B1)) & np.uint64(M)
    x ^= np.uint64((seed + site * 0x85EBCA77) & M)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(M)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(M)
    x ^= x >> np.uint64(16)
    u = (x >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return ~(u < np.float32(p))
