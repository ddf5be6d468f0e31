"""The hand-built Parquet images of test_parquet_images_cpu.py and test_parquet_images_gpu.py, built with pq_images.py.

One case is one column; a file holds many columns, so the GPU test decodes hundreds of cases in a handful of calls.
Every column's `doc` names the constant or branch of k_pq_snappy / k_pq_decode (mcr_parquet.hpp) it aims at, in the
names of pq_images.py: BATCH 64, IN_WIN 4096 (kInWin) with LOOKAHEAD 136, RING 32768 (kRing), REACH 28608
(kRing - kBatchOut), FLUSH 8192 (kFlush), DECODE_THREADS 256.

Each file function returns (image, page table, columns) and is built once per process."""
from __future__ import annotations

import functools

import numpy as np

from pq_images import (BATCH, BIT_PACKED, DATA, DICT, DOUBLE, FLOAT, FLUSH, INDEX, INT32, INT64, NONE, PLAIN, PLAIN_DICT, REACH,
                       RING, RLE_DICT, SNAPPY, STRUCTS, Chunk, Column, Opts, Page, build_file, data_page, dict_column,
                       dict_entries, hybrid, lit_header, rnd, snappy, snappy_column, tags_for, unknown_fields, uvarint)

TYPES = (INT32, INT64, FLOAT, DOUBLE)
SMALL_ROWS = 1100          # > 8200 / 8: the largest output of the small Snappy cases
BIG_ROWS = 13800           # 110 400 bytes: a 64-byte source 100 000 back that spans an 8 KB mark, plus what follows


class Seeds:
    def __init__(self, base):
        self.n = base

    def __call__(self):
        self.n += 1
        return self.n


def lit(n, sd, nb=None):
    return ("lit", rnd(n, sd()), nb) if nb is not None else ("lit", rnd(n, sd()))


def lone(sd, n=70):
    """A literal that never fits a batch (header + n > BATCH): the batch before it ends in front of it and the next one
    starts right behind it -- how the plans below put an element at a chosen byte of its batch."""
    assert n + 2 > BATCH
    return lit(n, sd)


def small_lits(total, sd, lo=20, hi=60):
    """`total` bytes as literals that fit a batch (the in-batch literal path, ring -> flush)."""
    rng = np.random.default_rng(sd())
    out = []
    while total:
        n = min(int(rng.integers(lo, hi + 1)), total)
        out.append(lit(n, sd))
        total -= n
    return out


def mixed(n_tokens, sd, produced):
    """A random legal plan: literals of 1..70 bytes (some with non-minimal headers) and copies of every tag."""
    rng = np.random.default_rng(sd())
    out = []
    for _ in range(n_tokens):
        if produced < 8 or rng.random() < 0.45:
            n = int(rng.integers(1, 71))
            nb = None
            if rng.random() < 0.2:
                nb = int(rng.integers(max(1, (n - 1).bit_length() + 7 >> 3), 5))
            out.append(lit(n, sd, nb))
        else:
            n = int(rng.integers(1, 65))
            off = int(rng.integers(1, min(produced, 70000) + 1)) if rng.random() < 0.5 else int(rng.integers(1, min(produced, 100) + 1))
            out.append(("copy", int(rng.choice(tags_for(off, n))), off, n))
        produced += n
    return out


def retag(tokens, tag):
    """The same plan with its tag-2 copies sent through `tag`."""
    return [("copy", tag, t[2], t[3]) if t[0] == "copy" and t[1] == 2 and tag in tags_for(t[2], t[3]) else t for t in tokens]


def lead_to(s, sd):
    """A literal of exactly s input bytes (header included): the next element starts at byte s of the batch."""
    if s - 1 <= 60:
        return lit(s - 1, sd, 0)
    return lit(s - 2, sd, 1)


# ---- Snappy: the small file --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def snappy_small():
    sd = Seeds(1000)
    cols = []

    def add(name, toks, doc, **kw):
        cols.append(snappy_column(name, toks, SMALL_ROWS, doc, seed=sd(), **kw))

    # literal lengths, minimal headers; alone at the head of the stream and behind a 3-byte literal
    for L in (1, 59, 60, 61, 62, 63, 64, 65, 255, 256, 257):
        doc = f"literal of {L} bytes, minimal header: L < 60 inline | nb = L - 59 extra bytes; header + L <= BATCH in the batch, else the lone-literal path"
        add(f"lit{L}", [lit(L, sd)], doc)
        add(f"lit{L}_behind3", [lit(3, sd), lit(L, sd)], doc)
    add("lit10_nb2", [lit(10, sd, 2)], "non-minimal length: 10 bytes in nb = 2 (`v &= (1 << 8 nb) - 1`)")
    add("lit70_nb4", [lit(70, sd, 4)], "non-minimal length: 70 bytes in nb = 4 (no mask; hdr = 5; lone literal > BATCH)")
    add("lit10_nb1_3_4", [lit(10, sd, 1), lit(10, sd, 3), lit(10, sd, 4), lit(60, sd, 1)], "nb = 1, 3, 4 inside one batch")
    # lone literals on either side of 64 bytes at every residue of the output position
    for r in range(16):
        for L, nb in ((60, 4), (64, 1), (65, None), (200, None)):
            toks = ([lit(r, sd)] if r else []) + [lit(L, sd, nb)]
            add(f"lone{L}_op{r}", toks,
                f"lone literal of {L} bytes at output position {r} mod 16: len <= BATCH goes LDS window -> ring, longer goes "
                "input -> global + ring with a head of (16 - op % 16) % 16 bytes, 16-byte body, tail")
    # every element kind starting at batch bytes 59..63: its header straddles the batch, the walk stops in front of it
    kinds = {"lit1": lambda: lit(7, sd, 0), "lit2": lambda: lit(7, sd, 1), "lit3": lambda: lit(7, sd, 2), "lit4": lambda: lit(7, sd, 3),
             "lit5": lambda: lit(7, sd, 4), "copy1": lambda: ("copy", 1, 20, 5), "copy2": lambda: ("copy", 2, 30, 9),
             "copy3": lambda: ("copy", 3, 40, 33)}
    for kname, mk in kinds.items():
        for s in range(59, 64):
            add(f"straddle_{kname}_at{s}", [lead_to(s, sd), mk(), lit(5, sd)],
                f"{kname} starting at byte {s} of a BATCH: `pos + il > 64` ends the walk, the element opens the next batch")
    # copies: offsets around 1..8 (lane % of), 63 | 64 | 65 against lengths 1..64 (of == len), through every tag that can
    for off in (1, 2, 3, 4, 7, 8, 63, 64, 65):
        for tag in (1, 2, 3):
            toks = [lone(sd, 72)]
            for n in range(1, 65):
                if tag in tags_for(off, n):
                    toks += [("copy", tag, off, n), lit(1 + n % 3, sd)]
            add(f"copy_off{off}_tag{tag}", toks,
                f"copies at offset {off}, every length tag {tag} can express: `of < len` -> lane % of, the equality of == len, hdr = {[0, 2, 3, 5][tag]}")
    # source position against the batch (step 4a: independent copies at once | step 4b: in stream order)
    scen = {
        "one_indep": ([lone(sd, 100), ("copy", 2, 50, 20), lit(5, sd), lone(sd)],
                      "exactly one independent copy in a batch: `im & (im - 1)` is 0, it goes through 4b"),
        "many_indep": ([lone(sd, 100), ("copy", 2, 90, 10), lit(3, sd), ("copy", 1, 40, 8), ("copy", 2, 100, 64), lit(2, sd), lone(sd)],
                       "three independent copies in a batch: step 4a"),
        "src_ends_at_op": ([lone(sd, 100), ("copy", 2, 60, 30), lit(4, sd), ("copy", 2, 54, 20), lone(sd)],
                           "second copy at opos = op + 34 with a source ending exactly at op: `opos - off + olen <= op` holds, 4a"),
        "src_ends_past_op": ([lone(sd, 100), ("copy", 2, 70, 10), ("copy", 2, 60, 30), lit(4, sd), ("copy", 2, 63, 20), lone(sd)],
                             "third copy's source ends one byte past op (the first copy's first output byte): 4b behind 4a"),
        "src_is_the_byte_at_op": ([lone(sd, 100), ("copy", 2, 70, 10), ("copy", 2, 60, 30), lit(4, sd), ("copy", 2, 44, 1), lone(sd)],
                                  "a 1-byte copy of the byte AT op, which the first copy of the batch writes: `<= op` is exact, 4b"),
        "first_src_ends_at_op": ([lone(sd, 100), ("copy", 2, 20, 20), ("copy", 2, 64, 44), lone(sd)],
                                 "first copy of the batch with off == len: its source ends at op; the second one's too"),
        "first_overlaps": ([lone(sd, 100), ("copy", 2, 19, 20), ("copy", 2, 90, 10), ("copy", 2, 80, 10), lone(sd)],
                           "first copy overlaps its own output by one byte (dependent) in front of two independent ones"),
        "chain": ([lone(sd, 100), ("copy", 2, 30, 16), ("copy", 2, 16, 16), ("copy", 2, 8, 24), lone(sd)],
                  "a copy whose source is the previous copy's output in the same batch, then an overlapping one over that"),
        "interleaved": ([lone(sd, 100)] + [("copy", 2, 80, 8), ("copy", 2, 8, 8)] * 3 + [lit(3, sd), ("copy", 2, 11, 8), lone(sd)],
                        "independent and dependent copies interleaved in one batch: 4a for the former, then 4b in order"),
    }
    for name, (toks, doc) in scen.items():
        add(f"batch_{name}_tag2", toks, doc)
        add(f"batch_{name}_tag3", retag(toks, 3), doc + " (tag 3)")
    # output sizes around FLUSH with an element crossing the mark
    add("out8", [lit(8, sd)], "n_out = 8: one flush of a head only")
    add("out16", [lit(5, sd), ("copy", 2, 5, 11)], "n_out = 16: one flush of exactly one 16-byte vector, no head or tail")
    add("out8184", small_lits(8150, sd) + [("copy", 2, 100, 34)], "n_out = FLUSH - 8: final flush(op) short of the mark")
    add("out8192", small_lits(8160, sd) + [("copy", 2, 100, 32)], "n_out = FLUSH: the last element ends on the mark")
    add("out8200_copy", small_lits(8180, sd) + [("copy", 2, 77, 20)], "n_out = FLUSH + 8: a copy crosses the 8 KB mark")
    add("out8200_lit", small_lits(8180, sd) + [lit(20, sd)], "n_out = FLUSH + 8: an in-batch literal crosses the 8 KB mark")
    add("out8200_lone", [lit(8000, sd), lit(200, sd)], "n_out = FLUSH + 8: a lone long literal crosses the mark (flushed = op + len)")
    # the last element of the stream against its batch (an element is at least two bytes: lane 1 is the earliest end)
    add("last_ends_lane1", [lone(sd, 71), lit(1, sd)], "the final batch is one 2-byte element: avail = 2, the walk ends at pos = 2")
    add("last_ends_lane63", [lone(sd, 70), lit(30, sd), ("copy", 2, 9, 7), lit(29, sd)],
        "the final batch is exactly BATCH bytes and its last element ends at lane 63")
    # a few of them again as DOUBLE (f64 output; any bit pattern, NaN payloads included, must pass through)
    add("f64_copy_off8", [lone(sd, 72)] + [x for n in range(1, 65) for x in (("copy", 2, 8, n), lit(1 + n % 3, sd))],
        "copies at offset 8 into a DOUBLE column", type_=DOUBLE)
    add("f64_lit257", [lit(257, sd)], "literal of 257 bytes into a DOUBLE column", type_=DOUBLE)
    add("f64_lit61_v2", [lit(3, sd), lit(61, sd)], "DOUBLE, data page v2 under Snappy", type_=DOUBLE, v2=True)
    return build_file(cols) + (cols,)


# ---- Snappy: the big file ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def snappy_big():
    sd = Seeds(5000)
    cols = []

    def add(name, toks, doc, **kw):
        cols.append(snappy_column(name, toks, BIG_ROWS, doc, seed=sd(), **kw))

    for L in (65535, 65536, 65537):
        add(f"lit{L}", [lit(L, sd)], f"literal of {L} bytes (nb = {2 if L <= 65536 else 3}), longer than RING: the lone path wraps the ring twice")
    add("lit65536_behind3", [lit(3, sd), lit(65536, sd)], "the same at output position 3: head of 13 bytes")
    # streams longer than one input window; the page header's pad sweeps the payload over every 16-byte alignment
    for p in range(16):
        s1, s2 = Seeds(6000), Seeds(7000)          # the same two streams at every pad
        a = [lit(3947, s1)]
        add(f"window_edge_pad{p}", a + mixed(500, s1, 3947),
            f"pad {p}: a lone literal of 3950 input bytes opens the stream, so the next batch sits at ip - win = 3950 + (address of "
            "the first element) % 16 -- "
            "on both sides of the `ip + LOOKAHEAD > win + IN_WIN` refill (3960) over the sweep; then 500 random elements", pad=p)
        add(f"window_mixed_pad{p}", mixed(1200, s2, 0),
            f"pad {p}: 1200 random elements, several IN_WIN refills at whatever element the window ends in", pad=p)
    # far copies: 64 bytes whose source spans the first 8 KB mark, twice in one batch and once alone
    for off in (REACH - 1, REACH, REACH + 1, RING - 1, RING, RING + 1, 65535, 65536, 100000):
        for tag in (2, 3):
            if tag not in tags_for(off, 64):
                continue
            P = off + FLUSH - 32                    # source = [8160, 8224)
            toks = small_lits(10000, sd)
            left = P - 10000
            while left:
                n = min(3000, left)
                toks.append(lit(n, sd))
                left -= n
            toks += [("copy", tag, off, 64), ("copy", tag, off, 64), lit(5, sd), lone(sd), ("copy", tag, off, 64), lit(4, sd), lone(sd)]
            # ... and once behind 960 bytes of the same batch's own output, which have taken ring slots by then: a source
            # more than RING - 960 back is gone from the ring whatever the test on `of` says
            toks += [("copy", 2, 8, 64)] * 15 + [("copy", tag, off, 64), lit(3, sd)]
            add(f"far_off{off}_tag{tag}", toks,
                f"offset {off} against REACH {REACH} / RING {RING}: `off <= kRing - kBatchOut` picks ring or flush + read-back; "
                "two such copies in one batch (4a when within REACH), one alone, one behind 960 bytes of its own batch's output; "
                "the first source spans the 8 KB mark at 8192")
    add("f64_far_off32768", small_lits(10000, sd) + [lit(3000, sd)] * 11 + [("copy", 2, RING, 64)] * 2, "offset RING into a DOUBLE column", type_=DOUBLE)
    s1 = Seeds(6000)
    add("f64_window_edge", [lit(3947, s1)] + mixed(500, s1, 3947), "the window-edge stream into a DOUBLE column", type_=DOUBLE, pad=5)
    return build_file(cols) + (cols,)


# ---- dictionary pages --------------------------------------------------------------------------------------------------
WIDTH_ROWS = 77


def width_runs(lim, rng):
    """24 packed values (3 full groups), two RLE runs, 28 packed values (4 groups, 4 of the last used): 77 values below lim."""
    a = rng.integers(0, lim, 24).tolist()
    a[0], a[23], a[5] = lim - 1, lim - 1, 0
    b = rng.integers(0, lim, 28).tolist()
    b[27] = lim - 1
    return [("packed", a), ("rle", 20, lim - 1), ("rle", 5, 0), ("packed", b)]


@functools.lru_cache(maxsize=None)
def dict_widths():
    rng = np.random.default_rng(11)
    cols = []
    k = 0
    for bw in range(33):
        for dn in (1, 2, 3, 300):
            k += 1
            type_ = TYPES[k % 4]
            lim = min(dn, 1 << bw)
            cols.append(dict_column(f"bw{bw}_dict{dn}", type_, dict_entries(dn, type_, k), [(bw, width_runs(lim, rng), WIDTH_ROWS)],
                                    f"bit width {bw} (mask `bw == 32 ? ~0 : (1 << bw) - 1`, RLE value in {(bw + 7) // 8} bytes) over a "
                                    f"dictionary of {dn}: indices up to {lim - 1}; last group with 4 of 8 used"))
    for w in range(13):
        dn = 1 << w
        type_ = TYPES[w % 4]
        cols.append(dict_column(f"full_dict_w{w}", type_, dict_entries(dn, type_, 500 + w), [(w, width_runs(dn, rng), WIDTH_ROWS)],
                                f"dictionary of exactly 2^{w} entries at width {w}: entries 0 and {dn - 1} used (`idx >= dn` must not fire)"))
    for u in range(1, 8):
        type_ = TYPES[u % 4]
        runs = [("rle", WIDTH_ROWS - 8 - u, 3), ("packed", rng.integers(0, 20, 8 + u).tolist())]
        cols.append(dict_column(f"last_group_{u}_used", type_, dict_entries(20, type_, 600 + u), [(5, runs, WIDTH_ROWS)],
                                f"last bit-packed group with {u} of 8 values used: `cnt = min(groups * 8, nv - done)`"))
    for u in (1, 7):
        runs = [("rle", WIDTH_ROWS - 8 - u, 3), ("packed", rng.integers(0, 20, 8 + u).tolist(), None, "cut")]
        cols.append(dict_column(f"last_group_{u}_used_cut", DOUBLE, dict_entries(20, DOUBLE, 700 + u), [(5, runs, WIDTH_ROWS)],
                                "the last run cut short of its padded bytes: `(cnt * bw + 7) / 8` bytes suffice (doubtful case)"))
    return cols


def file_of(cols, **kw):
    return build_file(cols, **kw) + (cols,)


@functools.lru_cache(maxsize=None)
def dict_widths_file():
    return file_of(dict_widths())


RUN_GROUPS = (1, 2, 31, 32, 33)
RUN_COUNTS = (1, 2, 255, 256, 257, 8191, 8192)


def long_runs(lim, rng):
    """Bit-packed runs of 1, 2, 31, 32, 33 groups and RLE runs of 1, 2, 255, 256, 257, 8191, 8192 alternating, a
    3-value group last.  31 | 32 | 33 groups are 248 | 256 | 264 values around DECODE_THREADS; RLE headers take 1, 2 and
    (8192 << 1) 3 varint bytes."""
    runs = []
    for i, c in enumerate(RUN_COUNTS):
        g = RUN_GROUPS[i] if i < len(RUN_GROUPS) else 1
        v = rng.integers(0, lim, 8 * g).tolist()
        v[0], v[-1] = lim - 1, lim - 1
        runs += [("packed", v), ("rle", c, int(rng.integers(0, lim)) if c != 256 else lim - 1)]
    runs.append(("packed", [lim - 1, 0, lim - 1]))
    return runs, sum(RUN_COUNTS) + 8 * (sum(RUN_GROUPS) + 2) + 3


@functools.lru_cache(maxsize=None)
def dict_runs_file():
    rng = np.random.default_rng(12)
    cols = []
    for bw, dn, type_, kw in ((1, 2, INT32, {}), (5, 20, DOUBLE, {}), (13, 5000, INT64, {}), (20, 300, FLOAT, {}), (32, 3, DOUBLE, {}),
                              (9, 400, DOUBLE, dict(codec=SNAPPY)), (7, 100, INT64, dict(codec=SNAPPY, optional=True, v2=True)),
                              (3, 8, FLOAT, dict(optional=True))):
        runs, n = long_runs(min(dn, 1 << bw), rng)
        cols.append(dict_column(f"runs_bw{bw}_{type_}" + "".join(f"_{a}" for a in kw), type_, dict_entries(dn, type_, 800 + bw),
                                [(bw, runs, n)], f"alternating run lengths at width {bw}: run headers of 1, 2 and 3 varint bytes, "
                                "packed runs across DECODE_THREADS, `done` not a multiple of 8 between runs", **kw))
    return file_of(cols)


MIXED_ROWS = 500


@functools.lru_cache(maxsize=None)
def dict_mixed_file():
    rng = np.random.default_rng(13)
    cols = []

    def runs(lim, n):
        a = rng.integers(0, lim, n - 100).tolist()
        return [("rle", 100, lim - 1), ("packed", a)]

    k = 0
    for type_ in TYPES:
        for codec in (NONE, SNAPPY):
            for v2 in (False, True):
                k += 1
                tail = dict_entries(250, type_, 900 + k)
                cols.append(dict_column(f"fallback_{type_}_{codec}_{int(v2)}", type_, dict_entries(37, type_, 950 + k), [(6, runs(37, 250), 250)],
                                        "a dictionary chunk that falls back to PLAIN: dictionary page, RLE_DICTIONARY page, PLAIN page; "
                                        + ("Snappy: the dictionary page is compressed too" if codec else "stored: no page is compressed"),
                                        codec=codec, v2=v2, optional=bool(k % 2), plain_tail=tail))
    for type_ in (INT64, DOUBLE):
        ent = dict_entries(300, type_, 990 + type_)
        pages = [(9, runs(300, 200), 200), (12, runs(300, 150), 150), (16, runs(300, 150), 150)]
        cols.append(dict_column(f"three_pages_{type_}", type_, ent, pages, "three data pages of different widths on one compressed dictionary", codec=SNAPPY))
        cols.append(dict_column(f"plain_dictionary_{type_}", type_, ent, pages, "PLAIN_DICTIONARY (encoding 2) on the dictionary and the data pages",
                                enc=PLAIN_DICT, optional=True))
        cols.append(dict_column(f"no_dict_offset_{type_}", type_, ent, pages, "no dictionary_page_offset: data_page_offset points at the dictionary page",
                                dict_offset="absent"))
        cols.append(dict_column(f"zero_dict_offset_{type_}", type_, ent, pages, "dictionary_page_offset = 0 (`m.dict_off > 0`)", dict_offset="zero",
                                codec=SNAPPY))
    c = dict_column("index_page_between", DOUBLE, dict_entries(50, DOUBLE, 77), [(6, runs(50, 250), 250), (6, runs(50, 250), 250)],
                    "an INDEX page between two data pages: walked over by open() (doubtful case)")
    c.chunks[0].pages.insert(2, Page(INDEX, 0, 0, b"\x00" * 16))
    cols.append(c)
    return file_of(cols)


@functools.lru_cache(maxsize=None)
def two_row_groups_file():
    """Two row groups of different sizes, two columns: every chunk has its own dictionary; one column's second chunk is PLAIN."""
    rng = np.random.default_rng(14)
    a1 = dict_column("a", INT64, dict_entries(10, INT64, 1), [(4, [("packed", rng.integers(0, 10, 100).tolist())], 100)], "", codec=SNAPPY)
    a2 = dict_column("a", INT64, dict_entries(300, INT64, 2), [(9, [("rle", 7, 299), ("packed", rng.integers(0, 300, 30).tolist())], 37)], "", codec=SNAPPY)
    b1 = dict_column("b", DOUBLE, dict_entries(4, DOUBLE, 3), [(2, [("packed", rng.integers(0, 4, 100).tolist())], 100)], "", optional=True)
    tail = dict_entries(37, DOUBLE, 4)
    b2 = Column("b", DOUBLE, True, [Chunk(NONE, [data_page(tail.tobytes(), 37, PLAIN, True, False, False)])], tail)
    cols = [Column("a", INT64, False, a1.chunks + a2.chunks, np.concatenate([a1.values, a2.values]),
                   "two chunks, each with a dictionary of its own: `dict` restarts per chunk, row_off carries over"),
            Column("b", DOUBLE, True, b1.chunks + b2.chunks, np.concatenate([b1.values, b2.values]), "dictionary chunk, then a PLAIN chunk")]
    return build_file(cols) + (cols,)


# ---- definition levels -------------------------------------------------------------------------------------------------
LEVEL_ROWS = 8 * 257 + 3     # 258 groups when bit-packed: two rounds of DECODE_THREADS; the last group has 3 of 8 used


def level_plans(n):
    ones = lambda k: [1] * k      # noqa: E731
    return {
        "rle2": [("rle", 5, 1), ("rle", n - 5, 1)],
        "rle_many": [("rle", 1, 1)] * 9 + [("rle", n - 9, 1)],
        "packed": [("packed", ones(n))],
        "mix": [("rle", 3, 1), ("packed", ones(64)), ("rle", 100, 1), ("packed", ones(n - 167))],
        "packed_then_rle": [("packed", ones(8)), ("rle", n - 8, 1)],
        "rle_then_packed": [("rle", n - 11, 1), ("packed", ones(11))],
        "rle_count_beyond": [("rle", 100, 1), ("rle", 100000, 1)],
    }


# A bit-packed LEVEL run cut short of the groups its header declares is not here: pyarrow refuses it ("Number of decoded
# rep / def levels do not match num_values in page header"), so it is dropped as the issue allows; the cut-short run of
# dictionary indices (dict_widths: last_group_*_used_cut) is read by pyarrow and stays.
DOUBTFUL_LEVELS = ("rle_count_beyond",)


@functools.lru_cache(maxsize=None)
def levels_file():
    n = LEVEL_ROWS
    cols = []
    k = 0
    for pname, plan in level_plans(n).items():
        for v2 in (False, True):
            for codec in (NONE, SNAPPY):
                k += 1
                type_ = TYPES[k % 4]
                vals = dict_entries(n, type_, 1200 + k)
                doc = (f"definition levels `{pname}` on a {'v2' if v2 else 'v1'} page, {n} values (not a multiple of 8): the zero padding of "
                       "a partial last group is masked (`(1 << (cnt - g * 8)) - 1`), RLE counts are clipped to the values left"
                       + (" (doubtful case)" if pname in DOUBTFUL_LEVELS else ""))
                name = f"lv_{pname}_{'v2' if v2 else 'v1'}_{codec}"
                if k % 3 == 0:       # dictionary-encoded values behind the levels
                    rng = np.random.default_rng(k)
                    c = dict_column(name, type_, vals[:40], [(6, [("packed", rng.integers(0, 40, n).tolist())], n)], doc, codec=codec,
                                    optional=True, v2=v2)
                    pg = c.chunks[0].pages[1]
                    body = pg.body if v2 else pg.body[4 + len(hybrid([("rle", n, 1)], 1)):]
                    c.chunks[0].pages[1] = data_page(body, n, RLE_DICT, True, codec == SNAPPY, v2, k, level_runs=plan)
                    cols.append(c)
                else:
                    pg = data_page(vals.tobytes(), n, PLAIN, True, codec == SNAPPY, v2, k, level_runs=plan)
                    cols.append(Column(name, type_, True, [Chunk(codec, [pg])], vals, doc))
    for flag, name in ((False, "false"), (None, "absent"), (True, "true")):
        for optional in (False, True):
            k += 1
            vals = dict_entries(n, DOUBLE, 1300 + k)
            pg = data_page(vals.tobytes(), n, PLAIN, optional, True, True, k, level_runs=level_plans(n)["mix"], is_compressed=flag)
            cols.append(Column(f"v2_is_compressed_{name}_{int(optional)}", DOUBLE, optional, [Chunk(SNAPPY, [pg])], vals,
                               f"data page v2 under a Snappy chunk with is_compressed {name}: `comp = SNAPPY && (!v2 || v2_compressed)`"))
    return file_of(cols)


NULL_ROWS = 8 * 257 + 7      # the last bit-packed group has 7 of 8 used


@functools.lru_cache(maxsize=None)
def null_images():
    """[(name, image, position of the null)]: one real null at each position of the partial last group, v1 and v2."""
    out = []
    n = NULL_ROWS
    for v2 in (False, True):
        for pos in range(7):
            lv = [1] * n
            at = n - 7 + pos
            lv[at] = 0
            vals = dict_entries(n - 1, DOUBLE, 1400 + pos)
            pg = data_page(vals.tobytes(), n, PLAIN, True, False, v2, level_runs=[("rle", 8, 1), ("packed", lv[8:])])
            col = Column("x", DOUBLE, True, [Chunk(NONE, [pg])], None, f"a null at position {pos} of the last group: PQE_NULLS through the partial mask")
            out.append((f"null_{'v2' if v2 else 'v1'}_pos{pos}", build_file([col])[0], at))
    return out


# ---- refusals on the device --------------------------------------------------------------------------------------------
def _snappy_refusal(tokens, n_values, preamble=None, usize=None):
    stream, _ = snappy(tokens, check=False, preamble=uvarint(8 * n_values) if preamble is None else preamble)
    usize = 8 * n_values if usize is None else usize
    pg = Page(DATA, n_values, PLAIN, b"\x00" * usize, stream)
    return build_file([Column("x", INT64, False, [Chunk(SNAPPY, [pg])], None)])[0]


def _dict_refusal(body, n_values, dn=5):
    ent = dict_entries(dn, INT64, 1)
    pages = [Page(DICT, dn, PLAIN, ent.tobytes()), Page(DATA, n_values, RLE_DICT, body)]
    return build_file([Column("x", INT64, False, [Chunk(NONE, pages)], None)])[0]


@functools.lru_cache(maxsize=None)
def refusal_images():
    """[(name, image, message, the guard in mcr_parquet.hpp that refuses it before any load or store uses the bad value)]"""
    sd = Seeds(9000)
    S, R, D = "corrupt Snappy stream", "corrupt RLE / bit-packed runs", "dictionary index out of range"
    return [
        ("copy_offset_0", _snappy_refusal([lit(16, sd), ("copy", 2, 0, 8)], 3), S,
         "k_pq_snappy batch validation `type != 0 && (off == 0 || off > opos)`, ahead of steps 3 and 4"),
        ("copy_offset_beyond_produced", _snappy_refusal([lit(16, sd), ("copy", 2, 17, 8)], 3), S,
         "k_pq_snappy batch validation `off > opos` (17 > 16)"),
        ("copy_offset_beyond_produced_tag3", _snappy_refusal([lit(16, sd), ("copy", 3, 1 << 31, 8)], 3), S,
         "k_pq_snappy batch validation `off > opos`, a 4-byte offset with the top bit set"),
        ("literal_past_stream_in_batch", _snappy_refusal([lit(16, sd), ("raw", lit_header(8) + rnd(4, 1))], 3), S,
         "k_pq_snappy batch validation `ip + lane + ilen > n_in`"),
        ("literal_past_stream_lone", _snappy_refusal([lit(16, sd), ("raw", lit_header(104) + rnd(50, 2))], 15), S,
         "k_pq_snappy lone literal `len > n_in - ip`, ahead of its loads"),
        ("output_overrun_in_batch", _snappy_refusal([lit(16, sd), ("copy", 2, 16, 16)], 3), S,
         "k_pq_snappy batch validation `opos + olen > n_out`"),
        ("output_overrun_lone", _snappy_refusal([lit(16, sd), lit(104, sd)], 3), S,
         "k_pq_snappy lone literal `len > n_out - op`, ahead of its stores"),
        ("preamble_differs", _snappy_refusal([lit(24, sd)], 4, preamble=uvarint(24)), S,
         "k_pq_snappy `uni(ulen) != n_out`, ahead of everything"),
        ("bit_width_33", _dict_refusal(bytes([33]) + hybrid([("rle", 16, 1)], 33), 16), R, "k_pq_decode `bw > 32`"),
        ("rle_count_0", _dict_refusal(bytes([3]) + hybrid([("rle", 8, 1), ("rle", 0, 1), ("rle", 8, 1)], 3), 16), R,
         "k_pq_decode RLE run `cnt0 == 0`"),
        ("packed_groups_0", _dict_refusal(bytes([3]) + hybrid([("rle", 8, 1)], 3) + b"\x01" + hybrid([("rle", 8, 1)], 3), 16), R,
         "k_pq_decode bit-packed run `groups == 0`"),
        ("rle_index_equals_dict_count", _dict_refusal(bytes([3]) + hybrid([("rle", 8, 1), ("rle", 8, 5)], 3), 16), D,
         "k_pq_decode RLE run `idx >= dn`, ahead of the dictionary load"),
        ("packed_index_equals_dict_count", _dict_refusal(bytes([3]) + hybrid([("packed", [0, 1, 2, 3, 4, 5, 4, 3] + [1] * 8)], 3), 16), D,
         "k_pq_decode bit-packed run `idx >= dn`: that value's dictionary load and store are skipped"),
    ]


# ---- host-only images: the Thrift reader -------------------------------------------------------------------------------
def host_columns(n_cols=4):
    """Small columns of every page kind, for files whose subject is the footer and the page headers."""
    rng = np.random.default_rng(21)
    n = 40
    cols = []
    for k in range(n_cols):
        type_ = TYPES[k % 4]
        if k % 3 == 0:
            c = dict_column(f"c{k}", type_, dict_entries(9, type_, k), [(4, [("rle", 8, 8), ("packed", rng.integers(0, 9, 32).tolist())], n)], "",
                            codec=SNAPPY if k % 2 else NONE, optional=True, v2=bool(k % 4 == 0))
        else:
            vals = dict_entries(n, type_, 30 + k)
            c = Column(f"c{k}", type_, bool(k % 2), [Chunk(SNAPPY if k % 2 else NONE, [
                data_page(vals[:25].tobytes(), 25, PLAIN, bool(k % 2), bool(k % 2), k % 3 == 2, k),
                data_page(vals[25:].tobytes(), 15, PLAIN, bool(k % 2), bool(k % 2), k % 3 == 2, k + 1)])], vals)
        for pg in c.chunks[0].pages:
            pg.crc, pg.stats = True, pg.kind != DICT
        cols.append(c)
    return cols


@functools.lru_cache(maxsize=None)
def host_images():
    """{name: (image, page table, columns)}: long-form ids, unknown fields of every Thrift type in each struct, a schema of
    20 columns (long list header), crc + statistics in the page headers (host_columns sets them everywhere)."""
    out = {"plain": build_file(host_columns()) + (host_columns(),),
           "long_ids": build_file(host_columns(), Opts(long_ids=True)) + (host_columns(),),
           "wide_schema": build_file(host_columns(20)) + (host_columns(20),),
           "unknown_everywhere_long_ids": build_file(host_columns(), Opts(True, {s: unknown_fields() for s in STRUCTS})) + (host_columns(),)}
    for s in STRUCTS:
        out[f"unknown_in_{s}"] = build_file(host_columns(), Opts(False, {s: unknown_fields()})) + (host_columns(),)
    return out


def bit_packed_levels_image():
    """A v1 page of an OPTIONAL column whose definition levels use the deprecated BIT_PACKED encoding: no 4-byte length,
    ceil(n / 8) bytes.  (image, values)"""
    n = 21
    vals = dict_entries(n, DOUBLE, 5)
    lv = bytes([0xFF, 0xFF, 0xFF])                   # 21 ones and padding of ones: the same in either bit order
    pg = Page(DATA, n, PLAIN, lv + vals.tobytes(), def_encoding=BIT_PACKED)
    return build_file([Column("x", DOUBLE, True, [Chunk(NONE, [pg])], vals)])[0], vals


def gpu_files():
    """Every image the GPU test decodes and compares with pyarrow: {name: (image, page table, columns)}."""
    out = {"snappy_small": snappy_small(), "snappy_big": snappy_big(), "dict_widths": dict_widths_file(), "dict_runs": dict_runs_file(),
           "dict_mixed": dict_mixed_file(), "two_row_groups": two_row_groups_file(), "levels": levels_file()}
    out.update({f"host_{k}": v for k, v in host_images().items() if k in ("unknown_everywhere_long_ids", "wide_schema")})
    return out
