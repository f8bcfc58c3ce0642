"""Every member of struct pg_ctx (poolgen_amd/csrc/pg_common.h) has a row in the "Carried state" table of tests/DISPATCH_COVERAGE.md
that names who writes it, who reads it and the test that covers it (or `not state`), and every row names a member: the next cached
field cannot arrive without someone deciding which test owns it.  No GPU."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "poolgen_amd" / "csrc" / "pg_common.h"
TABLE = ROOT / "tests" / "DISPATCH_COVERAGE.md"


def struct_members(text):
    body = re.search(r"struct pg_ctx \{\n(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    body = re.sub(r"\{[^{}]*\}", "", body)                     # brace initialisers: {0}, {true, true}
    while re.search(r"<[^<>]*>", body):
        body = re.sub(r"<[^<>]*>", "", body)                   # template arguments: DevBuf<void, true>
    names = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        for piece in stmt.split(","):
            piece = re.sub(r"=.*$", "", piece)                 # initialiser
            piece = re.sub(r"\[[^\]]*\]", "", piece).strip()   # array extent
            m = re.search(r"([A-Za-z_]\w*)$", piece)
            assert m, f"cannot read a member name out of {stmt!r}"
            names.append(m.group(1))
    return names


def table_rows(text):
    sec = re.search(r"^## Carried state[^\n]*\n(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert sec, "tests/DISPATCH_COVERAGE.md has no section 'Carried state'"
    rows = {}
    for line in sec.group(1).splitlines():
        m = re.match(r"\| `(\w+)` \|(.*)\|\s*$", line)
        if m:
            cells = [c.strip() for c in m.group(2).split("|")]
            assert m.group(1) not in rows, f"{m.group(1)} has two rows"
            rows[m.group(1)] = cells
    return rows


def test_parser_reads_every_form_of_declaration():
    sample = ("struct pg_ctx {\n    int a = -1;\n    int b = 0, c = -1; // x, y\n    DevBuf<void, true> d;\n    const double *e = nullptr;\n"
              "    bool f[2] = {true, true};   // ...\n    std::vector<double> g;    // n x k\n    double h[PG_K_COUNT] = {0};\n};\n")
    assert struct_members(sample) == list("abcdefgh")


def test_every_member_of_the_context_has_a_row_and_every_row_a_member():
    members = struct_members(HEADER.read_text())
    assert len(members) == len(set(members)) and len(members) > 40 and {"ws", "spec_valid", "rows_next", "comm_rank"} <= set(members)
    rows = table_rows(TABLE.read_text())
    missing = [m for m in members if m not in rows]
    stale = [r for r in rows if r not in members]
    assert not missing, f"members of struct pg_ctx without a row in the 'Carried state' table: {missing}"
    assert not stale, f"rows of the 'Carried state' table without a member of struct pg_ctx: {stale}"
    for name, cells in rows.items():
        assert len(cells) == 3 and all(cells), f"{name}: a row needs 'written by', 'read by' and a test (or `not state`)"
        assert cells[2] == "not state" or "test_" in cells[2] or "state::" in cells[2], f"{name}: the last cell names no test"
    for name in ("device", "cus", "err", "prof", "ev_pending", "ev_free", "prof_ms", "prof_n"):
        assert rows[name][2] == "not state", name


def test_named_context_state_tests_exist():
    """the `state::` names of the table are functions of tests/test_gpu_context_state.py"""
    src = (ROOT / "tests" / "test_gpu_context_state.py").read_text()
    defined = set(re.findall(r"^def (test_\w+)\(", src, re.M))
    rows = table_rows(TABLE.read_text())
    for name, cells in rows.items():
        for ref in re.findall(r"state::(test_\w+?)(?=[`\[\s*]|$)", cells[2]):
            if ref.endswith("_"):                             # `state::test_large_then_small_*`: a family of tests
                assert any(d.startswith(ref) for d in defined), (name, ref)
            else:
                assert ref in defined, (name, ref)
