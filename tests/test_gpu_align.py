"""fqh_align_scores on the GPU, bit-exact against tests/align_model.py: scores, end positions, the FQH_FLAG_ADAPTER bit, the
count, the gather of the records without a hit, argument checks, short / long / empty inputs, chunked use with lead bytes,
a buffer over 4 GiB, and the same result twice on the caller's stream."""
import numpy as np
import pytest

import align_model as am
import fuzzgen

pytestmark = pytest.mark.gpu

PARAMS = [(1, 0, 8, 1), (1, 0, 5, 1), (2, -3, 5, 2), (1, -1, 1, 1), (127, -127, 127, 0)]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g
    yield torch, g.load_package()
    # the 4.5 GiB buffer and the rest go back to the driver: later modules find the allocator as they would without this one
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def mutate(rng, frag):
    f = bytearray(frag)
    for _ in range(int(rng.integers(0, 4))):
        op = int(rng.integers(0, 3))
        p = int(rng.integers(0, len(f) + 1))
        if op == 0 and p < len(f):
            f[p] = int(rng.choice(list(b"ACGTN")))
        elif op == 1:
            f[p:p] = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 4))).astype(np.uint8))
        elif len(f) > 1:
            del f[p: p + int(rng.integers(1, 4))]
    return bytes(f)


def planted_file(rng, query, nrec, maxlen):
    """Records whose seq() holds a prefix, a suffix or an internal piece of the query, mutated (substitutions, insertions,
    deletions), between random bases; CRLF on some."""
    out = []
    for i in range(nrec):
        a, b = sorted(int(x) for x in rng.integers(0, len(query) + 1, 2))
        kind = i % 3
        frag = query[:b] if kind == 0 else query[a:] if kind == 1 else query[a:b]
        frag = mutate(rng, frag) if rng.random() < 0.7 else frag
        room = max(0, maxlen - len(frag))
        pre = bytes(rng.choice(list(b"ACGT"), int(rng.integers(0, room // 2 + 1))).astype(np.uint8))
        post = bytes(rng.choice(list(b"ACGT"), int(rng.integers(0, room // 2 + 1))).astype(np.uint8))
        seq = pre + frag + post
        nl = b"\r\n" if rng.random() < 0.1 else b"\n"
        out.append(b"@p%d" % i + nl + seq + nl + b"+" + nl + b"I" * len(seq) + nl)
    return b"".join(out)


def records(fqref, data):
    res, idx = fqref.index(data)
    assert res.status == 0
    return [fqref.accessors(data, row)[1] for row in idx]


class Loaded:
    """A file on the device, scanned and indexed."""

    def __init__(self, torch, pkg, data, lead=0):
        dev = torch.device("cuda:0")
        self.torch, self.pkg = torch, pkg
        self.ctx = pkg.Ctx(0, stream=torch.cuda.current_stream().cuda_stream)
        self.mem = torch.zeros(lead + len(data) + 64, dtype=torch.uint8, device=dev)
        if data:
            self.mem[lead: lead + len(data)].copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        self.ptr = self.mem.data_ptr() + lead
        self.len = len(data)
        s, _, _ = self.ctx.scan(self.ptr, self.len, True)
        assert s.parse_status == 0
        self.n = s.n_records
        self.idx = torch.zeros(max(1, self.n) * 24, dtype=torch.uint8, device=dev)
        if self.n:
            self.ctx.index_records(self.idx.data_ptr(), self.n)

    def align(self, query, params, threshold, flags=None, base_offset=0):
        torch = self.torch
        n = max(1, self.n)
        score = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
        end = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
        count = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")   # ADDED to
        match, mismatch, go, ge = params
        self.ctx.align_scores(self.ptr, self.len, self.idx.data_ptr(), self.n, query, match, mismatch, go, ge, threshold,
                              score.data_ptr(), end.data_ptr(), None if flags is None else flags.data_ptr(), count.data_ptr(),
                              base_offset=base_offset)
        torch.cuda.synchronize()
        return (score.cpu().numpy()[: self.n].astype(np.int64), end.cpu().numpy()[: self.n].view(np.uint32),
                int(count.cpu().numpy()[0]) - 5)


def check(loaded, seqs, query, params, threshold, with_flags=False):
    exp_s, exp_e = am.align_scores(seqs, query, *params)
    flags = None
    if with_flags:
        flags = loaded.torch.zeros(max(1, loaded.n), dtype=loaded.torch.uint8, device="cuda:0")
        loaded.ctx.record_flags(loaded.ptr, loaded.len, loaded.idx.data_ptr(), loaded.n, flags.data_ptr())
        before = flags.cpu().numpy()[: loaded.n].copy()
    s, e, c = loaded.align(query, params, threshold, flags)
    assert np.array_equal(s, exp_s), np.flatnonzero(s != exp_s)[:10]
    assert np.array_equal(e, exp_e), np.flatnonzero(e != exp_e)[:10]
    hit = exp_s > threshold
    assert c == int(hit.sum())
    if with_flags:
        after = flags.cpu().numpy()[: loaded.n]
        assert np.array_equal(after & 3, before & 3) and not (before & 4).any()
        assert np.array_equal((after & 4) != 0, hit)
    return exp_s, hit, flags


@pytest.mark.parametrize("maxlen", [17, 150, 300])
@pytest.mark.parametrize("params", PARAMS)
def test_fuzzed_files_with_planted_adapter(fqref, env, maxlen, params):
    torch, pkg = env
    rng = np.random.default_rng(maxlen * 31 + sum(params))
    data = fuzzgen.valid_file(rng, 600, maxlen=maxlen, crlf=maxlen == 150) + planted_file(rng, am.ADAPTER, 900, maxlen) \
        + fuzzgen.valid_file(rng, 300, maxlen=maxlen)
    seqs = records(fqref, data)
    L = Loaded(torch, pkg, data)
    assert L.n == len(seqs) == 1800
    thr = (10 if params[1] == 0 else 6) * params[0]
    exp, hit, flags = check(L, seqs, am.ADAPTER, params, thr, with_flags=True)
    assert exp.max() >= params[0] * 29 and exp.min() < exp.max()   # planted fragments: scores spread up to m * match
    assert 0 < hit.sum() < len(seqs)
    res, idx = fqref.index(data)
    expect = b"".join(data[int(r[0]): int(r[0]) + int(r[4]) + 1] for r, h in zip(idx, hit) if not h)
    out = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda:0")
    st, ns, nb = L.ctx.gather_records(L.ptr, L.len, L.idx.data_ptr(), L.n, flags.data_ptr(), pkg.FLAG_ADAPTER, 0,
                                      out.data_ptr(), out.numel())
    assert (st, ns, nb) == (pkg.OK, int((~hit).sum()), len(expect))
    assert out.cpu().numpy()[:nb].tobytes() == expect


@pytest.mark.parametrize("qlen", [1, 2, 17, 33, 58, 63, 64])
def test_query_lengths(fqref, env, qlen):
    torch, pkg = env
    rng = np.random.default_rng(900 + qlen)
    query = (am.ADAPTER + b"GATTACA")[:qlen]
    data = planted_file(rng, query, 700, 150) + fuzzgen.valid_file(rng, 300, maxlen=150)
    seqs = records(fqref, data)
    L = Loaded(torch, pkg, data)
    for params in ((2, -3, 5, 2), (1, 0, 8, 1)):
        check(L, seqs, query, params, max(1, qlen // 2))


def test_argument_ranges(env):
    torch, pkg = env
    L = Loaded(torch, pkg, b"@r\nACGT\n+\nIIII\n")
    ok = dict(match=1, mismatch=0, gap_open=8, gap_extend=1)
    bad = [dict(query=b""), dict(query=b"A" * 65), dict(match=0), dict(match=128), dict(mismatch=-128),
           dict(mismatch=2, match=1), dict(gap_extend=-1), dict(gap_extend=9, gap_open=8), dict(gap_open=128, gap_extend=1)]
    for b in bad:
        kw = dict(ok, query=b"ACGT")
        kw.update(b)
        with pytest.raises(pkg.FqhError) as e:
            L.ctx.align_scores(L.ptr, L.len, L.idx.data_ptr(), L.n, kw["query"], kw["match"], kw["mismatch"],
                               kw["gap_open"], kw["gap_extend"], 10)
        assert e.value.status == pkg.E_ARG, b
    # the edges of the ranges are accepted
    for q, m, x, go, ge in ((b"A" * 64, 127, -127, 127, 127), (b"A", 1, 1, 0, 0)):
        L.ctx.align_scores(L.ptr, L.len, L.idx.data_ptr(), L.n, q, m, x, go, ge, 0)
    torch.cuda.synchronize()


def test_kilobase_reads_among_short_ones_empty_and_single(fqref, env):
    torch, pkg = env
    rng = np.random.default_rng(77)
    parts = []
    for i, L in enumerate([36, 5000, 36, 36, 20000, 36, 0, 36]):
        seq = bytearray(rng.choice(list(b"ACGT"), L).astype(np.uint8))
        if L >= 5000:
            for p in (100, L // 2, L - 60):
                seq[p: p + 58] = mutate(rng, am.ADAPTER)[:58].ljust(58, b"A")
        parts.append(b"@k%d\n" % i + bytes(seq) + b"\n+\n" + b"#" * L + b"\n")
    data = b"".join(parts)
    seqs = records(fqref, data)
    check(Loaded(torch, pkg, data), seqs, am.ADAPTER, (2, -3, 5, 2), 20)
    check(Loaded(torch, pkg, parts[1]), seqs[1:2], am.ADAPTER, (1, 0, 8, 1), 10)   # a single record
    check(Loaded(torch, pkg, parts[6]), [b""], am.ADAPTER, (1, 0, 8, 1), 10)       # a single empty one
    Lz = Loaded(torch, pkg, b"")                                                       # n = 0
    assert Lz.n == 0
    s, e, c = Lz.align(am.ADAPTER, (1, 0, 8, 1), 10)
    assert c == 0


def test_chunks_with_lead_bytes_add_up_to_the_whole_file(fqref, env):
    """Pieces scanned with the carry of the one before; the record across a cut is kept in front of the next piece (its lead
    bytes) and scored with the piece it ends in, at base_offset = the piece's file offset."""
    torch, pkg = env
    rng = np.random.default_rng(5)
    data = planted_file(rng, am.ADAPTER, 3000, 150) + fuzzgen.valid_file(rng, 1000, maxlen=300)
    seqs = records(fqref, data)
    exp_s, _ = am.align_scores(seqs, am.ADAPTER, 1, 0, 8, 1)
    dev = torch.device("cuda:0")
    ctx = pkg.Ctx(0, stream=torch.cuda.current_stream().cuda_stream)
    LEAD = 4096
    cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, len(data)), 9, replace=False)) + [len(data)]
    carry, tail, got_scores = None, b"", []
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    for a, b in zip(cuts[:-1], cuts[1:]):
        piece = data[a:b]
        assert len(tail) <= LEAD
        mem = torch.zeros(LEAD + len(piece) + 64, dtype=torch.uint8, device=dev)
        blob = tail + piece
        mem[LEAD - len(tail): LEAD + len(piece)].copy_(torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()))
        ptr = mem.data_ptr() + LEAD
        fin = b == len(data)
        s, nxt, _ = ctx.scan(ptr, len(piece), fin, carry)
        assert s.parse_status == 0
        base = carry.base_offset if carry is not None else 0
        assert base == a
        if s.n_records:
            idx = torch.zeros(s.n_records * 24, dtype=torch.uint8, device=dev)
            ctx.index_records(idx.data_ptr(), s.n_records)
            sc = torch.zeros(s.n_records, dtype=torch.int32, device=dev)
            ctx.align_scores(ptr, len(piece), idx.data_ptr(), s.n_records, am.ADAPTER, d_score=sc.data_ptr(),
                             d_count=count.data_ptr(), base_offset=base)
            got_scores.append(sc.cpu().numpy().astype(np.int64))
        tail = blob[len(blob) - s.tail_len:] if not fin else b""
        carry = nxt
    got = np.concatenate(got_scores)
    assert np.array_equal(got, exp_s)
    assert int(count.cpu()[0]) == int((exp_s > 10).sum())


def test_same_result_twice_on_the_callers_stream(fqref, env):
    torch, pkg = env
    rng = np.random.default_rng(11)
    data = planted_file(rng, am.ADAPTER, 4000, 150)
    L = Loaded(torch, pkg, data)
    with torch.cuda.stream(torch.cuda.Stream()):
        L.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        a = L.align(am.ADAPTER, (2, -3, 5, 2), 15)
        b = L.align(am.ADAPTER, (2, -3, 5, 2), 15)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and a[2] == b[2]
    exp_s, exp_e = am.align_scores(records(fqref, data), am.ADAPTER, 2, -3, 5, 2)
    assert np.array_equal(a[0], exp_s) and np.array_equal(a[1], exp_e)


def test_buffer_over_4_gib(env):
    """A synthetic file of 4.5 GiB (fqh_synth_fill); adapter fragments written into the sequence lines of a few thousand
    records on the device (same lengths, then fqh_invalidate); sampled records across the whole buffer, the planted ones and
    the last ones bit-exact against the model; the count equals the number of scores above the threshold."""
    torch, pkg = env
    free, _ = torch.cuda.mem_get_info()
    size = (9 << 29) + 12345
    if free < size + (2 << 30):
        pytest.fail("needs %d bytes of free device memory, has %d" % (size + (2 << 30), free))
    dev = torch.device("cuda:0")
    ctx = pkg.Ctx(0, stream=torch.cuda.current_stream().cuda_stream)
    d = torch.empty(size + 64, dtype=torch.uint8, device=dev)
    ctx.synth_fill(d.data_ptr(), 0, size)
    s, _, _ = ctx.scan(d.data_ptr(), size, True)
    assert s.parse_status in (0, pkg.E_TRUNCATED)
    n = s.n_records
    idx = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
    ctx.index_records(idx.data_ptr(), n)
    rows = idx.view(torch.int64).view(n, 3)

    def lines(sel):
        """-> (first sequence byte, seq() length before the trim) of the records sel (numpy), read from the index."""
        r = rows[torch.from_numpy(sel).to(dev)]
        hs = r[:, 1].contiguous().view(torch.int32).view(-1, 2).cpu().numpy().astype(np.int64)   # head, seq
        first = r[:, 0].cpu().numpy() + hs[:, 0] + 1
        return first, hs[:, 1] - hs[:, 0] - 1
    rng = np.random.default_rng(3)
    planted = np.unique(np.concatenate([rng.integers(0, n, 3000), [n - 1, n - 2]]))
    pfirst, plen = lines(planted)
    pos, val = [], []
    for k in range(len(planted)):
        s0, sl = int(pfirst[k]), int(plen[k])
        frag = mutate(rng, am.ADAPTER[int(rng.integers(0, 20)):])[: max(1, sl - 3)]
        p = int(rng.integers(0, max(1, sl - len(frag) + 1)))
        for t, ch in enumerate(frag):
            pos.append(s0 + p + t)
            val.append(ch)
    d[torch.tensor(pos, dtype=torch.int64, device=dev)] = torch.tensor(val, dtype=torch.uint8, device=dev)
    ctx.invalidate()
    score = torch.zeros(n, dtype=torch.int32, device=dev)
    end = torch.zeros(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    params = (2, -3, 5, 2)
    ctx.align_scores(d.data_ptr(), size, idx.data_ptr(), n, am.ADAPTER, *params, 20, score.data_ptr(), end.data_ptr(), None,
                     count.data_ptr())
    torch.cuda.synchronize()
    assert int(count.cpu()[0]) == int((score > 20).sum().cpu())
    sample = np.unique(np.concatenate([planted, rng.integers(0, n, 2000), np.arange(n - 50, n)]))
    ssel = torch.from_numpy(sample).to(dev)
    sfirst, slen = lines(sample)
    seqs = []
    for k in range(len(sample)):
        s0, sl = int(sfirst[k]), int(slen[k])
        seqs.append(am.trim_winline(d[s0: s0 + sl].cpu().numpy().tobytes()))
    exp_s, exp_e = am.align_scores(seqs, am.ADAPTER, *params)
    assert np.array_equal(score[ssel].cpu().numpy().astype(np.int64), exp_s)
    assert np.array_equal(end[ssel].cpu().numpy().view(np.uint32), exp_e)
    assert (exp_s[np.isin(sample, planted)] > 20).sum() > 1000
    assert int(rows[n - 1, 0].cpu()) > (1 << 32)
    ctx.close()
    del d, idx, rows, score, end, count
