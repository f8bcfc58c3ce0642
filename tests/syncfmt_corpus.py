"""Rows for the sync line formatter (pg_sync_format_rows_dev, pg_host_sync_format_rows): hand-built ones with the bytes they must
give written out as literals, and seeded generators for the shapes the tests need.  A `rows` dictionary has the arrays a parser
returns -- counts (k x n x 6 uint32), pos (uint64), ref (uint8), line_off (int64), chrom_len (int32) -- plus `slab`, the text
the line offsets point into."""
import numpy as np

# every digit count of a uint32, at both ends
COUNT_EDGES = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999,
               100000000, 999999999, 1000000000, 4294967295]
POS_EDGES = [0, 1, 9, 10, 2 ** 32 - 1, 2 ** 32, 9999999999, 10 ** 10, 10 ** 19 - 1, 10 ** 19, 2 ** 64 - 1]
NAME_LENGTHS = [0, 1, 15, 16, 17, 300]


def rows_of(slab, rows):
    """rows: [(line_off, chrom_len, pos, ref byte, [[six counts] per pool])]"""
    k = len(rows)
    n = len(rows[0][4]) if k else 1
    return {"slab": bytes(slab),
            "counts": np.array([r[4] for r in rows], dtype=np.uint64).astype(np.uint32).reshape(k, n, 6),
            "pos": np.array([r[2] for r in rows], dtype=np.uint64), "ref": np.array([r[3] for r in rows], dtype=np.uint8),
            "line_off": np.array([r[0] for r in rows], dtype=np.int64), "chrom_len": np.array([r[1] for r in rows], dtype=np.int32)}


# (name, rows, the bytes they must give): written by hand, not computed
LITERALS = [
    ("two_pools",
     rows_of(b"chr1\t55\tA\twhatever follows\n", [(0, 4, 55, ord("A"), [[0, 1, 2, 3, 4, 5], [10, 0, 0, 0, 0, 4294967295]])]),
     b"chr1\t55\tA\t0:1:2:3:4:5\t10:0:0:0:0:4294967295\n"),
    ("empty_name_zero_position",
     rows_of(b"", [(0, 0, 0, ord("N"), [[0, 0, 0, 0, 0, 0]])]),
     b"\t0\tN\t0:0:0:0:0:0\n"),
    ("largest_position_and_counts",
     rows_of(b"xxscaffold_12yy", [(2, 11, 2 ** 64 - 1, ord("t"), [[4294967295] * 6])]),
     b"scaffold_12\t18446744073709551615\tt\t4294967295:4294967295:4294967295:4294967295:4294967295:4294967295\n"),
    ("positions_around_two_to_the_32",
     rows_of(b"c", [(0, 1, 4294967295, ord("C"), [[1, 22, 333, 4444, 55555, 666666]]),
                    (0, 1, 4294967296, ord("G"), [[7777777, 88888888, 999999999, 1000000000, 10, 100]]),
                    (1, 0, 10000000000, ord("*"), [[9, 99, 999, 9999, 99999, 999999]])]),
     b"c\t4294967295\tC\t1:22:333:4444:55555:666666\n"
     b"c\t4294967296\tG\t7777777:88888888:999999999:1000000000:10:100\n"
     b"\t10000000000\t*\t9:99:999:9999:99999:999999\n"),
    ("the_reference_line_of_vcf_rs",                                     # tests/golden/vcf_literals.json, "sync_line"
     rows_of(b"chrA\t323723\t.\tC\tA,CCT",
             [(0, 4, 323723, ord("C"), [[0, 0, 7, 0, 1, 0], [0, 0, 5, 0, 2, 0], [2, 0, 4, 0, 1, 0], [1, 0, 7, 0, 0, 0], [5, 0, 6, 0, 2, 0],
                                        [0, 0, 7, 0, 1, 0], [0, 0, 5, 0, 1, 0], [4, 0, 5, 0, 0, 0], [0, 0, 9, 0, 0, 0], [3, 0, 23, 0, 10, 0]])]),
     b"chrA\t323723\tC\t0:0:7:0:1:0\t0:0:5:0:2:0\t2:0:4:0:1:0\t1:0:7:0:0:0\t5:0:6:0:2:0\t0:0:7:0:1:0\t0:0:5:0:1:0\t4:0:5:0:0:0\t0:0:9:0:0:0"
     b"\t3:0:23:0:10:0\n"),
    ("names_share_the_slab_and_a_tab_as_reference",
     rows_of(b"Chromosome1Chromosome2", [(11, 11, 7, 9, [[1, 0, 0, 0, 0, 0]] * 3), (0, 11, 8, 0x7f, [[0, 0, 0, 0, 0, 12]] * 3)]),
     b"Chromosome2\t7\t\t\t1:0:0:0:0:0\t1:0:0:0:0:0\t1:0:0:0:0:0\n"
     b"Chromosome1\t8\t\x7f\t0:0:0:0:0:12\t0:0:0:0:0:12\t0:0:0:0:0:12\n"),
]


def name_slab():
    """A slab with a name of every NAME_LENGTHS length at an offset of every residue mod 16, the last one in the last bytes of
    the slab: (slab, [(offset, length)])."""
    slab = bytearray()
    places = []
    k = 0
    for length in NAME_LENGTHS:
        for residue in range(16):
            while len(slab) % 16 != residue:
                slab += b"\t"                                            # (a byte no name holds: a copy that starts early or ends late shows)
            places.append((len(slab), length))
            slab += bytes(33 + (k + i) % 94 for i in range(length))      # printable, different from name to name
            k += 7
    slab += bytes(65 + i for i in range(17))                             # the last bytes of the slab: names that end exactly where it ends
    last = [(len(slab) - l, l) for l in (0, 1, 15, 16, 17)]
    return bytes(slab), places + last


def generated(n, rows, seed, digits=None, names=True):
    """`rows` rows of n pools.  Counts: edge values and random ones of every digit count mixed inside a pool (or all of `digits`
    digits); positions: the edges, then random ones of every length; ref: every byte value in turn; names: name_slab()'s places
    in turn (names=False: the empty name at offset 0 of a one-byte slab)."""
    rng = np.random.default_rng(seed)
    edges = np.array(COUNT_EDGES, dtype=np.uint64)
    if digits is None:
        nd = rng.integers(1, 11, size=(rows, n, 6))
        lo = np.where(nd == 1, 0, 10 ** (nd - 1)).astype(np.uint64)
        hi = np.minimum(10 ** nd.astype(np.uint64), np.uint64(2 ** 32)).astype(np.uint64)
        c = lo + (rng.random((rows, n, 6)) * (hi - lo).astype(np.float64)).astype(np.uint64)
        c = np.minimum(c, hi - 1)
        pick = rng.random((rows, n, 6)) < 0.3
        c = np.where(pick, edges[rng.integers(0, len(edges), size=(rows, n, 6))], c)
    else:
        lo, hi = (0 if digits == 1 else 10 ** (digits - 1)), min(10 ** digits, 2 ** 32)
        c = rng.integers(lo, hi, size=(rows, n, 6), dtype=np.uint64)
    pe = np.array(POS_EDGES, dtype=np.uint64)
    pos = rng.integers(0, 2 ** 63, size=rows, dtype=np.uint64) >> rng.integers(0, 63, size=rows).astype(np.uint64)
    pos[:len(pe)] = pe[:rows]
    ref = (np.arange(rows) % 256).astype(np.uint8)
    if names:
        slab, places = name_slab()
        idx = np.arange(rows) % len(places)
        off = np.array([places[i][0] for i in idx], dtype=np.int64)
        clen = np.array([places[i][1] for i in idx], dtype=np.int32)
    else:
        slab, off, clen = b"c", np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int32)
    return {"slab": slab, "counts": c.astype(np.uint32), "pos": pos, "ref": ref, "line_off": off, "chrom_len": clen}


ARRAYS = ("counts", "pos", "ref", "line_off", "chrom_len")


def args_of(rows):
    """the arguments of sync_format_host / syncfmt_ref.rows_text, in order"""
    return [rows[k] for k in ARRAYS] + [rows["slab"]]
