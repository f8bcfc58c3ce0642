"""Sync texts for the sync reader's tests: texts that parse, and texts at which the CLI's host parser throws, with the
(offset, reason) the library must report for them.  Reasons: pg_sync_reason (include/poolgen_hip.h)."""
import numpy as np

from sync_ref import E_COUNT, E_COUNT32, E_EMPTY, E_FIELDS, E_POOLS

GOOD = "1:2:3:4:5:6"


def line(chrom, pos, pools, ref="A"):
    return "\t".join([chrom, str(pos), ref] + list(pools)) + "\n"


def random_text(rng, n, lines, comment_every=0):
    """`lines` data lines of n pools with counts of every width, and the counts they hold (lines x n x 6)"""
    widths = np.array([0, 9, 10, 99, 100, 65535, 65536, 4294967295], dtype=np.uint64)
    counts = rng.integers(0, 300, size=(lines, n, 6)).astype(np.uint64)
    pick = rng.random(size=counts.shape) < 0.1
    counts[pick] = widths[rng.integers(0, len(widths), size=int(pick.sum()))]
    out = []
    for i in range(lines):
        if comment_every and i % comment_every == 0:
            out.append(f"# comment {i}\n")
        out.append(line(f"chr{i // 10}", 1000 + 7 * i, [":".join(str(int(x)) for x in counts[i, j]) for j in range(n)]))
    return "".join(out).encode(), counts.astype(np.uint32)


def corpus():
    """name -> (text, expect_n): texts that parse"""
    two = [GOOD, "0:0:0:0:0:0"]
    c = {}
    c["crlf_no_final_newline"] = ((line("c1", 5, two)[:-1] + "\r\n" + line("c1", 6, two)[:-1] + "\r\n" + line("c2", 7, two)[:-1] + "\r").encode(), 0)
    c["no_final_newline"] = ((line("c1", 5, two) + line("c1", 6, two)[:-1]).encode(), 0)
    c["comments_in_the_middle"] = (("#head\tx\n" + line("c1", 5, two) + "# a\tcomment\twith\ttabs\t1:2\n#\n" + line("c1", 6, two) + "#end").encode(), 0)
    c["bad_positions_are_skipped"] = ((line("c1", 1, two) + line("c1", "x", two) + line("c1", "+5", two) + line("c1", "-1", two) + line("c1", "", two)
                                       + line("c1", "1" * 20, two) + line("c1", "9" * 19, two) + line("c1", "12x", two) + "c1\tx\tA\n" + "c1\tx\t\n"
                                       + line("c1", "x", two + ["1:2"]) + line("c1", 2, two)).encode(), 0)
    c["leading_zeros"] = ((line("c1", "0005", ["01:002:0003:0:00:" + "0" * 18 + "7", "0:0:0:0:0:0000065536"])).encode(), 0)
    c["count_widths"] = ((line("c1", 5, ["0:9:10:65535:65536:4294967295", "4294967295:4294967294:1:0:0:0"])).encode(), 0)
    c["plus_signs"] = ((line("c1", 5, ["+1:+2:3:4:5:+6", GOOD])).encode(), 0)
    c["seven_and_eight_counts"] = ((line("c1", 5, [GOOD + ":7", GOOD + ":7:8"]) + line("c1", 6, [GOOD + ":99999999999", GOOD])).encode(), 0)
    c["one_pool"] = ((line("c1", 5, [GOOD]) + line("c1", 6, ["6:5:4:3:2:1"])).encode(), 0)
    c["first_line_bad_position_fixes_the_pools"] = ((line("c1", "x", two) + line("c1", 6, two) + line("c2", 7, two)).encode(), 0)
    c["only_comments"] = (b"#a\n#b\n", 0)
    c["only_skipped_lines"] = (line("c1", "x", two).encode(), 0)
    c["expect_n_good"] = ((line("c1", 5, two) + line("c1", 6, two)).encode(), 2)
    c["many_chromosomes"] = ("".join(line(f"chromosome_{i % 4}_{'x' * (i % 5)}", i + 1, two) for i in range(40)).encode(), 0)
    c["empty_chromosome_name"] = ((line("", 5, two) + line("c", 6, two)).encode(), 0)
    rng = np.random.default_rng(7)
    c["random_5_pools"] = (random_text(rng, 5, 50, comment_every=9)[0], 0)
    return c


def error_texts():
    """name -> (text, expect_n, offset, reason): texts that fail, and the first bad line"""
    two = [GOOD, "0:0:0:0:0:0"]
    ok = line("c1", 5, two)
    o = len(ok)
    e = {}
    e["empty_line"] = ((ok + "\n" + ok).encode(), 0, o, E_EMPTY)
    e["empty_first_line"] = (("\n" + ok).encode(), 0, 0, E_EMPTY)
    e["only_cr"] = ((ok + "\r\n" + ok).encode(), 0, o, E_EMPTY)
    e["only_cr_at_the_end"] = ((ok + "\r").encode(), 0, o, E_EMPTY)
    e["two_fields"] = ((ok + "c1\t5\n").encode(), 0, o, E_FIELDS)
    e["one_field"] = ((ok + "c1\n").encode(), 0, o, E_FIELDS)
    e["two_fields_bad_position"] = ((ok + "c1\tx\n").encode(), 0, o, E_FIELDS)
    e["three_fields"] = ((ok + "c1\t5\tA\n").encode(), 0, o, E_FIELDS)
    e["three_fields_first_line_bad_position"] = (("c1\tx\tA\n" + ok).encode(), 0, 0, E_FIELDS)     # skipped anywhere else
    e["five_counts"] = ((ok + line("c1", 6, ["1:2:3:4:5", GOOD])).encode(), 0, o, E_COUNT)
    e["empty_count"] = ((ok + line("c1", 6, [GOOD, "1::3:4:5:6"])).encode(), 0, o, E_COUNT)
    e["seventh_is_a_letter"] = ((ok + line("c1", 6, [GOOD + ":x", GOOD])).encode(), 0, o, E_COUNT)
    e["trailing_colon"] = ((ok + line("c1", 6, [GOOD + ":", GOOD])).encode(), 0, o, E_COUNT)
    e["count_above_u32"] = ((ok + line("c1", 6, [GOOD, "1:2:3:4:5:4294967296"])).encode(), 0, o, E_COUNT32)
    e["count_of_20_digits"] = ((ok + line("c1", 6, ["1" * 20 + ":2:3:4:5:6", GOOD])).encode(), 0, o, E_COUNT)
    e["letter_inside_a_count"] = ((ok + line("c1", 6, [GOOD, "1:2:3a:4:5:6"])).encode(), 0, o, E_COUNT)
    e["minus_sign"] = ((ok + line("c1", 6, [GOOD, "1:2:-3:4:5:6"])).encode(), 0, o, E_COUNT)
    e["one_pool_more"] = ((ok + line("c1", 6, two + [GOOD])).encode(), 0, o, E_POOLS)
    e["one_pool_fewer"] = ((ok + ok + line("c1", 6, [GOOD])).encode(), 0, 2 * o, E_POOLS)
    e["trailing_tab"] = ((ok + line("c1", 6, two)[:-1] + "\t\n").encode(), 0, o, E_POOLS)       # the empty third pool is not looked at
    e["trailing_tab_one_pool_fewer"] = ((ok + line("c1", 6, [GOOD])[:-1] + "\t\n").encode(), 0, o, E_COUNT)
    e["ends_in_the_middle_of_a_pool"] = ((ok + ok + line("c1", 6, two)[:-8]).encode(), 0, 2 * o, E_COUNT)
    e["ends_after_a_pool"] = ((ok + line("c1", 6, two)[:-13]).encode(), 0, o, E_POOLS)
    e["expect_n_wrong"] = ((ok + ok).encode(), 3, 0, E_POOLS)
    e["expect_n_wrong_first_line_skipped"] = ((line("c1", "x", two) + ok).encode(), 3, 0, E_POOLS)
    e["first_bad_line_of_several"] = ((ok + line("c1", 6, ["1:2:3:4:5:4294967296", GOOD]) + "\n" + "c1\n").encode(), 0, o, E_COUNT32)
    e["smallest_reason_of_a_line"] = ((ok + line("c1", 6, ["1:2:3:4:5:4294967296", "x", GOOD])).encode(), 0, o, E_COUNT)
    return e
