"""CPU checks of fqh_align_scores' definition (tests/align_model.py) and of its ABI surface: the vectorised model against
a cell-by-cell statement, hand-worked scores, and the new symbol declared in include/fastq_hip.h, exported by
libfastq_hip.so and bound in fastq-rs_amd/binding.py and rust/ffi.rs."""
import os
import re
import subprocess

import numpy as np
import pytest

import align_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = am.ADAPTER


def one(seq, query=Q, **kw):
    s, e = am.align_scores([seq], query, **kw)
    return int(s[0]), int(e[0])


@pytest.mark.parametrize("params", [(1, 0, 8, 1), (1, 0, 5, 1), (2, -3, 5, 2), (1, -1, 1, 1), (127, -127, 127, 0), (3, 1, 2, 2)])
def test_model_equals_cell_by_cell_statement(params):
    match, mismatch, go, ge = params
    rng = np.random.default_rng(sum(params) + 7 * go)
    for _ in range(6):
        m = int(rng.integers(1, 12))
        query = bytes(rng.choice(list(b"ACGT"), m).astype(np.uint8))
        seqs = []
        for _ in range(25):
            L = int(rng.integers(0, 30))
            s = bytearray(rng.choice(list(b"ACGTN"), L).astype(np.uint8))
            if L > m and rng.random() < 0.5:    # plant the query, mutated
                p = int(rng.integers(0, L - m + 1))
                s[p: p + m] = query
                for _ in range(int(rng.integers(0, 3))):
                    s[int(rng.integers(0, L))] = int(rng.choice(list(b"ACGT")))
            seqs.append(bytes(s))
        got_s, got_e = am.align_scores(seqs, query, match, mismatch, go, ge)
        for k, s in enumerate(seqs):
            assert (int(got_s[k]), int(got_e[k])) == am.align_one(s, query, match, mismatch, go, ge), (s, query, params)


def test_query_against_itself_scores_m_times_match():
    assert one(Q) == (len(Q), len(Q) - 1)
    assert one(Q, match=3) == (3 * len(Q), len(Q) - 1)
    assert one(b"TTTT" + Q + b"GG") == (len(Q), 4 + len(Q) - 1)


def test_one_mismatch():
    s = bytearray(Q)
    s[30] = ord("A") if s[30] != ord("A") else ord("C")
    # identity scores: one lost match; with a mismatch penalty the better of the two halves or the penalised whole
    assert one(bytes(s))[0] == len(Q) - 1
    assert one(bytes(s), match=2, mismatch=-3)[0] == max(2 * (len(Q) - 1) - 3, 2 * 30, 2 * (len(Q) - 31))


def test_single_insertion_and_deletion_cost_open_plus_extend():
    m = len(Q)
    for k in (1, 2, 3):
        ins = Q[:29] + b"G" * k + Q[29:]            # k extra read bytes: a gap in the query, E
        dele = Q[:29] + Q[29 + k:]                  # k query bytes missing from the read: a gap in the read, F
        for go, ge in ((5, 1), (3, 2), (2, 0)):
            cost = go + (k - 1) * ge
            expect_ins = max(m - cost, 29, m - 29)
            expect_del = max(m - k - cost, 29, m - 29 - k)
            assert one(ins, gap_open=go, gap_extend=ge)[0] == expect_ins, (k, go, ge)
            assert one(dele, gap_open=go, gap_extend=ge)[0] == expect_del, (k, go, ge)
    # gap_open 2 makes the gapped alignment the best one: it ends at the read's last adapter byte
    ins = Q[:29] + b"G" + Q[29:]
    assert one(ins, gap_open=2, gap_extend=1) == (len(Q) - 2, len(ins) - 1)


def test_empty_read_scores_zero():
    assert one(b"") == (0, am.END_NONE)
    assert one(b"", query=b"A") == (0, am.END_NONE)
    assert one(b"TTTT", query=b"A") == (0, am.END_NONE)


def test_carriage_return_is_trimmed_once():
    assert am.trim_winline(b"ACGT\r") == b"ACGT"
    assert am.trim_winline(b"ACGT\r\r") == b"ACGT\r"
    assert am.trim_winline(b"") == b""
    # the '\r' is not a base: "A\r" against query "\r" scores 0 once trimmed
    assert one(am.trim_winline(b"A\r"), query=b"\r") == (0, am.END_NONE)
    assert one(b"A\r", query=b"\r") == (1, 1)


def test_end_is_the_first_column_that_reaches_the_score():
    # two exact copies: the score is reached first at the end of the first copy
    assert one(b"ACGT" + b"TTTTTT" + b"ACGT", query=b"ACGT") == (4, 3)
    # a longer second hit wins
    assert one(b"ACGC" + b"CCCCCC" + b"ACGT", query=b"ACGT") == (4, 13)
    # single-byte query: the first matching byte
    assert one(b"TTGAG", query=b"G") == (1, 2)


def test_case_sensitive_and_arbitrary_bytes():
    assert one(b"acgt", query=b"ACGT") == (0, am.END_NONE)
    assert one(b"\x00\xff~", query=b"\xff~") == (2, 2)


def _declared():
    src = open(os.path.join(ROOT, "include", "fastq_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(fqh_[a-z0-9_]+)\s*\(", src)), src


def test_align_scores_is_declared_exported_and_bound():
    decl, src = _declared()
    assert "fqh_align_scores" in decl
    assert re.search(r"#define\s+FQH_ALIGN_MAX_QUERY\s+64\b", src)
    assert re.search(r"#define\s+FQH_FLAG_ADAPTER\s+4u\b", src)
    import __graft_entry__ as g
    pkg = g.load_package()
    if not os.path.exists(pkg.LIB_PATH):
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "fqh_align_scores" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "fqh_align_scores" in pkg.EXPORTS
    assert hasattr(pkg.Ctx, "align_scores")
    assert pkg.lib().fqh_align_scores.argtypes is not None and len(pkg.lib().fqh_align_scores.argtypes) == 17
    assert (pkg.ALIGN_MAX_QUERY, pkg.FLAG_ADAPTER, pkg.ADAPTER) == (64, 4, am.ADAPTER)
    rs = open(os.path.join(ROOT, "fastq-rs_amd", "rust", "ffi.rs")).read()
    assert re.search(r"pub fn fqh_align_scores\(", rs)
    assert re.search(r"const FQH_FLAG_ADAPTER: u8 = 4;", rs) and re.search(r"const FQH_ALIGN_MAX_QUERY: u32 = 64;", rs)


def test_align_count_binary_is_built():
    import __graft_entry__ as g
    g.load_package()
    host = os.path.join(ROOT, "fastq-rs_amd", "host")
    assert "bin/fastq_align_count" in open(os.path.join(host, "Makefile")).read()
    assert os.path.exists(os.path.join(host, "fastq_align_count.cpp"))
