"""bin/fastq_align_count, the twin of examples/alignment_count.rs: the count of records whose alignment score against the
adapter is above the threshold equals the model's (tests/align_model.py), whatever the piece size, for plain, gzip and
stdin input; a malformed file exits 101 with the reference's message and prints no count."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import align_model as am
import fuzzgen
from test_gpu_align import planted_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fastq-rs_amd", "host", "bin", "fastq_align_count")


@pytest.fixture(scope="module")
def tool():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    g.load_package()
    if not os.path.exists(BIN):
        g.build()
    return BIN


def run(args, stdin=None, timeout=300):
    return subprocess.run(["timeout", "-k", "10", str(timeout), BIN] + args, input=stdin, capture_output=True, timeout=timeout + 30)


def model_count(fqref, data, p):
    res, idx = fqref.index(data)
    assert res.status == 0
    seqs = [fqref.accessors(data, row)[1] for row in idx]
    s, _ = am.align_scores(seqs, am.ADAPTER, p["match"], p["mismatch"], p["gap_open"], p["gap_extend"])
    return int((s > p["threshold"]).sum())


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    rng = np.random.default_rng(2024)
    data = planted_file(rng, am.ADAPTER, 3000, 150) + fuzzgen.valid_file(rng, 2000, maxlen=150) \
        + planted_file(rng, am.ADAPTER[20:], 1000, 40)
    d = tmp_path_factory.mktemp("align")
    p = d / "small.fq"
    p.write_bytes(data)
    (d / "small.fq.gz").write_bytes(gzip.compress(data))
    return data, p


def flags_of(p):
    return ["--match", str(p["match"]), "--mismatch", str(p["mismatch"]), "--gap-open", str(p["gap_open"]),
            "--gap-extend", str(p["gap_extend"]), "--threshold", str(p["threshold"])]


def test_count_equals_model_default_and_doc_flags(fqref, tool, small):
    data, path = small
    want = model_count(fqref, data, am.EXAMPLE)
    r = run([str(path)])
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == want
    want_doc = model_count(fqref, data, am.DOC_EXAMPLE)
    r = run(flags_of(am.DOC_EXAMPLE) + [str(path)])
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == want_doc
    p = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2, threshold=30)
    want_p = model_count(fqref, data, p)
    assert 0 < want_p < want
    r = run(flags_of(p) + ["--adapter", am.ADAPTER.decode(), "--piece-mib", "1", str(path)])
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == want_p


def test_gzip_and_stdin_give_the_same_count(fqref, tool, small):
    data, path = small
    p = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2, threshold=30)
    want = model_count(fqref, data, p)
    r = run(flags_of(p) + [str(path) + ".gz"])
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == want
    r = run(flags_of(p) + ["-"], stdin=data)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == want
    r = run(flags_of(p), stdin=gzip.compress(data))
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == want


def test_pieces_of_one_mib_count_what_one_piece_counts(tool, tmp_path):
    rng = np.random.default_rng(99)
    block = planted_file(rng, am.ADAPTER, 4000, 150) + fuzzgen.valid_file(rng, 4000, maxlen=300)
    data = block * (24 * 2**20 // len(block) + 1)        # tens of MiB: every 1 MiB cut falls inside some record
    path = tmp_path / "big.fq"
    path.write_bytes(data)
    p = dict(match=2, mismatch=-3, gap_open=5, gap_extend=2, threshold=30)
    counts = []
    for piece in ("1", "3", "1024"):
        r = run(flags_of(p) + ["--piece-mib", piece, str(path)])
        assert r.returncode == 0, r.stderr
        counts.append(int(r.stdout))
    reps = len(data) // len(block)
    assert counts[0] == counts[1] == counts[2]
    assert counts[0] % reps == 0 and counts[0] > 0


@pytest.mark.parametrize("bad", [b"@r\nACGT\n+\nIII\n", b"@r\nACGT\n+\nIIII\nr2\nA\n+\nI\n", b"@r\nACGT\n-\nIIII\n"])
def test_malformed_file_exits_101_with_the_reference_message(fqref, tool, tmp_path, bad):
    import __graft_entry__ as g
    pkg = g.load_package()
    data = planted_file(np.random.default_rng(1), am.ADAPTER, 50, 150) + bad
    res, _ = fqref.index(data)
    assert res.status != 0
    path = tmp_path / "bad.fq"
    path.write_bytes(data)
    r = run([str(path), "--piece-mib", "1"])
    assert r.returncode == 101
    assert r.stdout == b""
    assert r.stderr.decode().strip() == "Invalid fastq file: " + pkg.strerror(res.status)
